/* sphx.h — C ABI of the MI355X-native DFSPH step loop (libsphx.so).
 *
 * This is the drop-in boundary behind yasph2d's `Solver` trait / particle-array surface.  Every entry point
 * cites the reference interface (path:line relative to the yasph2d repository root) it replaces.  The Rust-side
 * binding a maintainer would add (an `impl Solver for HipDfsphSolver` in src/sph/solver/) is shown in INTEGRATION.md.
 *
 * Conventions
 *   - plain pointers and sizes only; `float* xy` arrays are interleaved {x,y} pairs, i.e. exactly the memory of a
 *     `Vec<cgmath::Point2<f32>>` / `Vec<cgmath::Vector2<f32>>` (src/units.rs:2-4).
 *   - every call returns an `int` status (SPHX_OK == 0).  Nothing aborts or throws across the boundary: the places
 *     where the reference panics (dfsph.rs:223,378 `assert!(is_finite)`, neighborhood_search.rs:373 bounds panic,
 *     Duration::from_secs_f32 on non-finite input) become error codes; sphx_last_error() gives the text.
 *   - the caller owns every host pointer (borrowed for the duration of the call); the library owns all device memory.
 *   - one context = one caller thread at a time (mirrors `&mut self` of Solver::simulation_step, solver/mod.rs:17).
 *   - all device work runs on one HIP stream — the context's own, or the caller's (sphx_set_stream); calls that return host data
 *     synchronise it.  The only exception is the viewer feed's device-to-host copy, which has a stream of its own.
 *
 * What is the contract and what is scaffolding (the header has grown beyond the boundary SURVEY.md 8(b) asks for):
 *   STABLE — the drop-in boundary a Rust shim binds:
 *       lifecycle (sphx_default_params, sphx_create, sphx_destroy, sphx_last_error, sphx_abi_version), the particle-array
 *       surface (sphx_set_boundary, sphx_upload, sphx_append, sphx_remove, sphx_download*, sphx_num_*, sphx_view_*, sphx_sample_*, sphx_render*, sphx_state_*, sphx_track_*, sphx_download_by_id, sphx_particle_fields, sphx_fluid_stats, sphx_stats_*, sphx_query_radius, sphx_select, sphx_gauge_*, sphx_probe_*), the Solver trait (sphx_clear_cached,
 *       sphx_step_begin[_law], sphx_step_finish, sphx_wcsph_step_*), the same trait over a device list (sphx_multi_create[_rank],
 *       sphx_multi_destroy, sphx_multi_set_boundary, sphx_multi_upload, sphx_multi_clear_cached, sphx_multi_step_begin/finish,
 *       sphx_multi_simulation_step[s], sphx_multi_download, sphx_multi_sample_*, sphx_sample_merge, sphx_multi_query_radius, sphx_multi_select, sphx_query_merge, sphx_multi_gauge_levels, sphx_gauge_merge, sphx_multi_probe_*, sphx_multi_num_owned, sphx_multi_last_error, sphx_comm_ops) and
 *       the status / flag codes.
 *   INSPECTION — parity tests and tools, not on the hot path, may change with the data layout:
 *       sphx_update_neighborhood, sphx_update_densities, sphx_compute_alpha (the pieces benches/ drives), sphx_download_solver_state,
 *       sphx_download_neighbors, sphx_download_cells, sphx_grid_info, sphx_get_constants, sphx_last_flags, sphx_build_stats,
 *       sphx_multi_info, sphx_multi_tile_ctx, sphx_multi_tile_rects, sphx_multi_ghost_rings, sphx_multi_set_layout / _set_grid_layout, sphx_profile_*, sphx_synchronize,
 *       sphx_set_tiling_invariant (a comparison mode: a run that does not depend on how the domain is tiled).
 *   INTERNAL — the seam between the tile loop (csrc/sphx_tiles.cpp) and a tile's context, exported so that the tests can drive the
 *       same sub-steps from the reference implementation of that loop (tests/tiles_reference.py); no stability promise:
 *       sphx_reserve, sphx_tile_*, sphx_sub_*, sphx_set_stream, sphx_shm_*.
 *   HOST MIRROR — the C++ twin of the reference's host types (world, timer, solver object) for hosts without a Rust toolchain:
 *       sphx_world_*, sphx_timer_*, sphx_solver_*, sphx_duration_*.
 */
#ifndef SPHX_H
#define SPHX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SPHX_ABI_VERSION 5 /* 5: sphx_shm_allgather, sphx_tile_send_counts, sphx_multi_info_t.halo_bytes_{packed,sent} / .ownership_seconds (appended)
                            * 4: sphx_set_tiling_invariant
                            * 2: sphx_step_stats.remote_entries, sphx_multi_*, frame-loop calls, sphx_sub_regrid_{div,warm}, SPHX_FLAG_DENSE_CELL
                            * 3: sphx_comm_ops.abort, sphx_multi_info_t list statistics, sphx_shm_abort (and sphx_shm_open as a collective),
                            *    sphx_build_stats, sphx_sub_run_ahead, sphx_tile_carry_warmstart, sphx_tile_defer_advect, sphx_sub_predict_iteration, sphx_tile_band_packs,
                            *    sphx_multi_info_t.band_packs (was reserved)
                            * 5 (additive): sphx_params.viscosity_model / .fluid_viscosity (were reserved[0..1]; zero = XSPH, the behaviour
                            *    before), SPHX_VISCOSITY_*, sphx_get_viscosity
                            * 5 (additive): sphx_sample_points, sphx_sample_grid, sphx_sample_out, SPHX_SAMPLE_DEVICE_POINTERS
                            * 5 (additive): sphx_render, sphx_render_fit, sphx_render_view, sphx_render_out, SPHX_RENDER_*
                            * 5 (additive): sphx_multi_render, sphx_multi_render_layer, sphx_render_merge, sphx_render_layer, sphx_tile_render_layer,
                            *    sphx_tile_render_window
                            * 5 (additive): sphx_append, sphx_remove, sphx_rect, SPHX_REMOVE_*, sphx_solver_append, sphx_solver_remove
                            * 5 (additive): sphx_state_size / _save / _load / _digest / _save_file / _load_file, SPHX_STATE_*, sphx_timer_state,
                            *    sphx_timer_get_state / _set_state, sphx_solver_save / _load
                            * 5 (additive): sphx_multi_state_size / _save / _load / _digest / _save_file / _load_file, sphx_tile_state_pack / _fetch,
                            *    sphx_tile_upload_state, sphx_get_tiling_invariant, sphx_solver_multi_checkpoint / _restore
                            * 5 (additive): sphx_track_set / _fetch / _record / _get_status / _read, sphx_download_by_id, sphx_track_out,
                            *    sphx_track_status, SPHX_TRACK_*
                            * 5 (additive): sphx_particle_fields, sphx_fields_out, SPHX_FIELDS_DEVICE_POINTERS
                            * 5 (additive): sphx_fluid_stats, sphx_stats_record / _get_status / _read, sphx_stats_rec, sphx_stats_frame,
                            *    sphx_stats_status, SPHX_STATS_*
                            * 5 (additive): sphx_multi_append, sphx_multi_remove, sphx_tile_remove_mark / _fetch, sphx_tile_append,
                            *    sphx_tile_grow
                            * 5 (additive): sphx_multi_track_set / _fetch / _record / _get_status / _read, sphx_multi_download_by_id,
                            *    sphx_multi_track_out, sphx_track_merge, sphx_track_merge_frames, sphx_tile_track_install / _fetch_enqueue /
                            *    _fetch / _window_enqueue / _window_fetch / _record / _frame / _read
                            * 5 (additive): sphx_multi_sample_points, sphx_multi_sample_grid, sphx_multi_sample_out, sphx_sample_merge,
                            *    sphx_multi_tile_rects, sphx_multi_ghost_rings, sphx_tile_sample_points / _points_fetch / _window /
                            *    _window_fetch, SPHX_SAMPLE_FIELD_*
                            * 5 (additive): sphx_multi_particle_fields, sphx_multi_fields_out, sphx_tile_owned_count,
                            *    sphx_tile_particle_fields_enqueue / _fetch, SPHX_FIELD_*
                            * 5 (additive): sphx_surface_contour, sphx_contour_chain, sphx_contour_out, SPHX_CONTOUR_*
                            * 5 (additive): sphx_multi_surface_contour, sphx_multi_contour_out, sphx_contour_merge,
                            *    sphx_tile_contour_sample / _border_fetch / _cut / _fetch
                            * 5 (additive): sphx_query_radius, sphx_select, sphx_query_out, sphx_select_out, SPHX_QUERY_*, SPHX_SELECT_*
                            * 5 (additive): sphx_multi_query_radius, sphx_multi_select, sphx_query_merge, sphx_multi_query_out,
                            *    sphx_multi_select_out, sphx_tile_query_radius / _query_fetch / _select / _select_fetch, sphx_tile_query_part
                            * 5 (additive): sphx_gauge_levels, sphx_gauge_reduce, sphx_probe_record / _get_status / _read, sphx_gauge, sphx_gauge_rec,
                            *    sphx_probe_rec, sphx_probe_status, SPHX_GAUGE_*
                            * 5 (additive): sphx_multi_gauge_levels, sphx_gauge_merge, sphx_gauge_part, sphx_multi_probe_record / _get_status /
                            *    _read, sphx_tile_gauge_levels / _gauge_fetch, sphx_tile_probe_record / _due / _frame / _read */

/* ---- status codes ---- */
enum {
    SPHX_OK = 0,
    SPHX_ERR_INVALID_ARGUMENT = 1,
    SPHX_ERR_NO_DEVICE = 2,       /* no HIP device / HIP runtime error; the product has no CPU fallback */
    SPHX_ERR_HIP = 3,
    SPHX_ERR_NOT_READY = 4,       /* step called before upload / begin-finish out of order */
    SPHX_ERR_NONFINITE = 5,       /* dfsph.rs:223,378 assert!(avg.is_finite()) */
    SPHX_ERR_NEIGHBOR_PANIC = 6,  /* neighborhood_search.rs:373: 64 dynamic neighbours and a static hit (reference panics) */
    SPHX_ERR_CAPACITY = 7,        /* a capacity was exceeded (halo exchange buffer, sphx_reserve, 2^32 table entries) */
    SPHX_ERR_OUT_OF_DOMAIN = 8    /* a particle left the Morton domain the grid tables were sized for */
};

/* ---- stats.flags bits ---- */
enum {
    SPHX_FLAG_NEIGHBOR_CAP = 1u,            /* "particle has too many neighbors" (neighborhood_search.rs:361,376) */
    SPHX_FLAG_DENSITY_ITER_CAP = 2u,        /* "Density error correction canceled" (dfsph.rs:236-245) */
    SPHX_FLAG_DIVERGENCE_ITER_CAP = 4u,     /* "Divergence error correction canceled" (dfsph.rs:391-400) */
    SPHX_FLAG_WARMUP = 8u,                  /* this step ran the warm-up block (dfsph.rs:419-428) */
    SPHX_FLAG_STRAY_PARTICLES = 16u,        /* a particle moved more than a 64-cell block beyond the covered region in one step (a blow-up);
                                               it is kept, without neighbours, and the cell directory is re-covered before the next build */
    SPHX_FLAG_DENSE_CELL = 32u              /* a cell held more than 4096 particles (a collapse to a point, or strays parked together):
                                               their order INSIDE that cell follows arrival, not the previous index — the stable rank
                                               costs occupancy^2 loads and would stall the GPU; everything else is unaffected */
};

/* sphx_params.viscosity_model: the ViscosityModel the DFSPH / WCSPH solver is generic over (src/sph/viscositymodel/,
 * DFSPHSolver<V> dfsph.rs:16-47, WCSPHSolver<V> wscsph.rs:14-42).  Zero is XSPH, so a zero-filled struct behaves as before. */
enum {
    SPHX_VISCOSITY_XSPH = 0,     /* XSPHViscosityModel (xsph.rs): xsph_epsilon */
    SPHX_VISCOSITY_PHYSICAL = 1  /* PhysicalViscosityModel (physical.rs): fluid_viscosity * m * Viscosity::laplacian / rho_j (viscosity.rs:44-46) */
};

/* kernel kinds for sphx_update_densities (src/sph/smoothing_kernel/) */
enum { SPHX_KERNEL_WENDLAND_C2 = 0, SPHX_KERNEL_POLY6 = 1, SPHX_KERNEL_SPIKY = 2 };

typedef struct sphx_ctx sphx_ctx;

/* Everything the reference hard-codes or derives from ConstantFluidProperties, as one POD.
 * sphx_default_params() fills the values of the reference app (main.rs:85-89, dfsph.rs:49-55, xsph.rs:14,
 * fluidparticleworld.rs:123, neighborhood_search.rs:478). */
typedef struct sphx_params {
    float smoothing_length;            /* h: DFSPHSolver::new(_, smoothing_length) dfsph.rs:43; also the search radius / cell size
                                          (fluidparticleworld.rs:118, neighborhood_search.rs:466) */
    float particle_mass;               /* ConstantFluidProperties::particle_mass() fluidparticleworld.rs:74-76 */
    float fluid_density;               /* rho0, fluidparticleworld.rs:70-72 */
    float particle_radius;             /* fluidparticleworld.rs:87-89 (CFL diameter = 2*radius, dfsph.rs:479) */
    float gravity[2];                  /* FluidParticleWorld::gravity, fluidparticleworld.rs:98,123 */
    float grid_min[2];                 /* GridProperties::grid_min, neighborhood_search.rs:478 */
    float xsph_epsilon;                /* XSPHViscosityModel::epsilon, xsph.rs:8,14 */
    float max_avg_density_error;       /* dfsph.rs:49 */
    uint32_t max_density_iterations;   /* dfsph.rs:50 */
    float max_divergence_error;        /* dfsph.rs:53 */
    uint32_t max_divergence_iterations;/* dfsph.rs:54 */
    uint32_t fixed_density_iterations; /* 0 = adaptive (reference behaviour); >0 = run exactly this many (parity/bench mode) */
    uint32_t fixed_divergence_iterations;
    int32_t device;                    /* HIP device ordinal */
    uint32_t list_span_limit;          /* neighbour-list layout (neighborhood_search.rs:262-273, README.md:12 "WIP"): lists are local to a
                                          workgroup of 256 Morton-consecutive particles — 16-bit slots of the record window the traversal
                                          kernels stage in LDS, plus a per-workgroup table of at most this many out-of-window neighbour
                                          entries.  0 = default (512, the table's capacity); SPHX_LISTS_32BIT = 32-bit global indices
                                          everywhere (traversals gather from global memory); smaller values only put more workgroups on
                                          that fallback (test aid).  Results never depend on it. */
    uint32_t viscosity_model;          /* SPHX_VISCOSITY_*; sphx_create rejects other values (SPHX_ERR_INVALID_ARGUMENT) */
    float fluid_viscosity;             /* PhysicalViscosityModel::fluid_viscosity (mu, Pa s), physical.rs:8,14: default 1.0016/1000 (water);
                                          main.rs:96 sets 0.01.  Only the physical model reads it; it must be finite (negative is accepted,
                                          as in the reference) */
    uint32_t reserved[1];
} sphx_params;
#define SPHX_LISTS_32BIT 0xFFFFFFFFu

/* Per-step report (the reference only println!s these; dfsph.rs:227-243,382-398). */
typedef struct sphx_step_stats {
    uint32_t density_iterations;       /* num_density_correction_iterations after the step (dfsph.rs:26) */
    uint32_t divergence_iterations;    /* num_divergence_correction_iterations (dfsph.rs:33) */
    uint32_t warmstart_density;        /* 1 if the kappa warm-start pass ran (dfsph.rs:199-205) */
    uint32_t warmstart_divergence;     /* 1 if the stiffness warm-start pass ran (dfsph.rs:354-360) */
    float avg_density_error;           /* last avg_density_error (dfsph.rs:221) */
    float avg_divergence;              /* last avg_divergence (dfsph.rs:376) */
    float dt_prev;                     /* dt the XSPH term used (dfsph.rs:433) */
    float dt;                          /* dt of prediction/solve/advect (dfsph.rs:478-480) */
    float vmax;                        /* sqrt(max |v + a*dt_prev|^2) handed to TimeManager (dfsph.rs:474-479) */
    uint32_t flags;                    /* SPHX_FLAG_* */
    uint32_t remote_entries;           /* of neighbor_entries: entries outside their workgroup's record window (they go through the
                                          workgroup's out-of-window table; byte accounting of the list layout) */
    uint64_t neighbor_entries;         /* sum of count_total over particles (length of the neighbour list buffer) */
} sphx_step_stats;

/* ---- lifecycle ---------------------------------------------------------------------------------------------- */
/* replaces DFSPHSolver::new (dfsph.rs:43-61) + the solver-owned part of FluidParticleWorld::new (fluidparticleworld.rs:104-127) */
int sphx_default_params(float smoothing_factor, float particle_density, float fluid_density, sphx_params* out);
int sphx_create(const sphx_params* params, sphx_ctx** out_ctx);
void sphx_destroy(sphx_ctx* ctx);
const char* sphx_last_error(const sphx_ctx* ctx); /* ctx may be NULL: returns the last creation error */
uint32_t sphx_abi_version(void);

/* ---- particle-array surface (fluidparticleworld.rs:11-23) ---------------------------------------------------- */
/* Particles::boundary_particles + boundary_changed=true (fluidparticleworld.rs:181-195); rebuilt lazily like :247-252 */
int sphx_set_boundary(sphx_ctx* ctx, const float* xy, uint32_t n);
/* Particles::positions / velocities (vel_xy may be NULL = zero).  Drops nothing cached: like the reference, caches are
 * rebuilt when the particle count differs from the cached arrays' length (dfsph.rs:419) or after sphx_clear_cached. */
int sphx_upload(sphx_ctx* ctx, const float* pos_xy, const float* vel_xy, uint32_t n);
/* Any pointer may be NULL.  Arrays are in the library's current (cell-sorted) order — the reference also re-sorts in
 * place every step (neighborhood_search.rs:121-140).  particle_id[i] = index the particle had in the last sphx_upload, or the id
 * sphx_append gave it since. */
int sphx_download(sphx_ctx* ctx, float* pos_xy, float* vel_xy, float* density, uint32_t* particle_id);
int sphx_download_boundary(sphx_ctx* ctx, float* xy, uint32_t* boundary_id);
/* Viewer feed (the app draws every particle at its position, coloured by |v|, main.rs:239-258): {x, y, |v|} of
 * every stride-th particle, packed on the solver stream and copied to pinned host memory on a separate stream, so the transfer
 * overlaps the following steps.  sphx_view_fetch returns the buffer of the latest request (3 floats per entry, valid until the next
 * request); wait = 0 polls (SPHX_ERR_NOT_READY while the copy is in flight). */
int sphx_view_request(sphx_ctx* ctx, uint32_t stride, uint32_t* out_count);
int sphx_view_fetch(sphx_ctx* ctx, int wait, const float** out_xys, uint32_t* out_count);
uint32_t sphx_num_particles(const sphx_ctx* ctx);  /* Particles::num_dynamic_particles  fluidparticleworld.rs:37 */
uint32_t sphx_num_boundary(const sphx_ctx* ctx);   /* Particles::num_boundary_particles fluidparticleworld.rs:41 */

/* ---- field sampling: density, fluid fraction and velocity at arbitrary points (an SPH "measure tool") -------------------------------
 * Kernel interpolation over the particles at query points, from the cell grids the latest neighbour build left on the device: one short
 * kernel, nothing added to the step.  The contract, for a query point q (fp32 x, y) and the kernel W of kind kernel_kind
 * (SPHX_KERNEL_*: the kinds sphx_update_densities takes; Wendland is the DFSPH kernel):
 *   Candidates: with (cx, cy) the cell of q, computed as for a particle (sat_u16((q - grid_min) * cell_inv), neighborhood_search.rs:52-58),
 *     the fluid particles of the 3x3 cells around (cx, cy), then the boundary particles of those cells; each in ascending device
 *     (cell-sorted) index, i.e. the order of sphx_download / sphx_download_boundary.  A particle the grid holds no cell for (a stray,
 *     SPHX_FLAG_STRAY_PARTICLES) contributes nothing, as in the neighbour build.
 *   Acceptance: dx = x_j.x - q.x, dy = x_j.y - q.y, d2 = dx*dx + dy*dy (unfused); accepted iff d2 <= radius_sq (radius_sq = h*h in fp32).
 *     Unlike the neighbour build there is no d2 > 1e-10 exclusion: a query point is not a particle, nothing at distance 0 is "self".
 *     w = W(d2, r) with r = sqrtf(d2) (correctly rounded): Wendland w_norm*(1-q)^2*(1-q)^2*(q+0.25) with q = min(w_hinv*r, 1),
 *     Poly6 p6_norm*d^3 with d = max(h*h - d2, 0), Spiky sp_norm*d^3 with d = max(h - r, 0), as sphx_update_densities evaluates them.
 *   Outputs (any subset; every sum starts at 0.0f and is accumulated in candidate order, one fp32 rounding per operation):
 *     density  = rho = rho + w*m over the fluid and then the boundary candidates, unclamped (the sum FluidParticleWorld::update_densities
 *                forms before its max(fluid_density), fluidparticleworld.rs:197-231);
 *     fraction = sum over fluid candidates of a_j, a_j = (m / rho_j) * w, rho_j = the density sphx_download returns for particle j:
 *                ~1 in the bulk, ~0.5 at the free surface, 0 away from the fluid;
 *     velocity = (sum a_j*v_j.x / fraction, sum a_j*v_j.y / fraction) (Shepard-normalised, v_j = sphx_download's velocity; the products
 *                a_j*v_j are summed, then divided once), (0, 0) where fraction == 0;
 *     count    = accepted fluid candidates (no cap: the build's 64-neighbour cap does not apply).
 *   A point far outside the domain or a non-finite one gets zeros and count 0 (a NaN coordinate saturates to cell 0 and fails every
 *   distance test); it never faults.
 * When a query is allowed: the cell grids and density[] must belong to the current positions — after sphx_step_finish, after
 * sphx_wcsph_step_finish (not after a step over zero fluid particles: it builds no grid), and after sphx_update_neighborhood followed by
 * sphx_update_densities.  After sphx_upload or sphx_set_boundary,
 * between a step_begin and its step_finish (either solver), after a failed step, or after a neighbour update without a density update the
 * call returns SPHX_ERR_NOT_READY and sphx_last_error says which step is missing.  A tile context (sphx_tile_*, sphx_multi_tile_ctx) is
 * refused with SPHX_ERR_INVALID_ARGUMENT: its arrays hold ghosts and miss the particles other tiles own.
 * No side effects: a query only reads (it does not touch the run-ahead pass, densities, lists, ids, SPHX_FLAG_* or sphx_last_flags); a run
 * with queries between its steps is bit-identical to the same run without them.
 * Argument errors (SPHX_ERR_INVALID_ARGUMENT, the message names the argument): out NULL or requesting no output, xy NULL with m > 0,
 * an unknown kernel_kind or flag bit; for the lattice dx / dy not finite or <= 0, x0 / y0 not finite, nx * ny >= 2^31.  m == 0 and
 * nx * ny == 0 are successful no-ops (once the arguments pass). */
enum { SPHX_SAMPLE_DEVICE_POINTERS = 1u }; /* xy and every output are device pointers on the context's device: the call is enqueued on the
                                              context's stream and returns without waiting (order it with sphx_synchronize / sphx_set_stream).
                                              Without it: host pointers; the call returns when the outputs are written (the library copies
                                              through a device scratch it grows on demand and frees in sphx_destroy). */
typedef struct sphx_sample_out {
    float* density;    /* [m] or NULL */
    float* fraction;   /* [m] or NULL */
    float* velocity;   /* [2m] interleaved xy, or NULL */
    uint32_t* count;   /* [m] or NULL */
} sphx_sample_out;
/* m points, xy interleaved.  They are processed in the caller's order, one lane each: pass large point sets SPATIALLY COHERENT (e.g. sorted
 * by cell) — neighbouring lanes then gather the same cells; random order costs several times more ("Sampling the fields"). */
int sphx_sample_points(sphx_ctx* ctx, const float* xy, uint32_t m, int kernel_kind, uint32_t flags, const sphx_sample_out* out);
/* The lattice point (ix, iy) is (x0 + (float)ix * dx, y0 + (float)iy * dy) in fp32 (unfused), output index iy * nx + ix (row 0 at y0,
 * the bottom).  Both calls share one device function for the walk of a point: sampling the lattice and sampling the same fp32 points
 * through sphx_sample_points give bit-identical outputs. */
int sphx_sample_grid(sphx_ctx* ctx, float x0, float y0, float dx, float dy, uint32_t nx, uint32_t ny, int kernel_kind,
                     uint32_t flags, const sphx_sample_out* out);

/* ---- free-surface extraction: the iso-contour of a sampled field, as directed segments (marching squares on the device) -------------
 * The dam-break papers plot the free-surface profile; a viewer draws a water line.  sphx_surface_contour samples a lattice, cuts the
 * contour `field == iso` out of it and returns the segments in a defined order, without the lattice crossing to the host;
 * sphx_contour_chain (host code) stitches segments into polylines.  The contract (every fp32 operation is rounded once, unfused):
 *   Lattice values: f[iy*nx+ix] is exactly what sphx_sample_grid returns for the chosen field (SPHX_CONTOUR_FIELD_FRACTION: fraction,
 *     SPHX_CONTOUR_FIELD_DENSITY: density) at that lattice, kernel_kind and state — the same device function, the same bits.
 *     out->values, when given, receives those bits.
 *   Inside test: b = (f >= iso) in fp32; a NaN value is outside.
 *   Cells: cell (ix, iy), 0 <= ix < nx-1, 0 <= iy < ny-1, has the nodes 0 = (ix, iy), 1 = (ix+1, iy), 2 = (ix+1, iy+1), 3 = (ix, iy+1)
 *     and the edges B (0-1), R (1-2), T (3-2), L (0-3).  Each edge is written a-b: a is the node with the lower lattice index
 *     iy*nx+ix, b the one with the higher, so the two cells that share an edge name it alike.
 *   Crossing point: an edge whose nodes differ in b has t = (iso - f_a) / (f_b - f_a) and the point
 *     p = (x_a + t*(x_b - x_a), y_a + t*(y_b - y_a)), with x_a, y_a the lattice coordinates of sphx_sample_grid
 *     (x0 + (float)ix*dx, y0 + (float)iy*dy).  Both cells that share an edge compute the same bits: the contour is watertight by bit
 *     equality.
 *   Segments: case c = b0 | b1<<1 | b2<<2 | b3<<3; cases 0 and 15 emit nothing.  A segment is directed with the inside on its left:
 *       1: B->L    2: R->B    4: T->R    8: L->T    3: R->L    6: T->B    12: L->R    9: B->T
 *      14: L->B   13: B->R   11: R->T    7: T->L
 *     Saddle cells (5 and 10): the centre ((f0+f1)+(f2+f3))*0.25f is inside iff it is >= iso.
 *       5, centre inside: B->R and T->L; outside: B->L and T->R.      10, centre inside: R->T and L->B; outside: R->B and L->T.
 *     Of the two segments of a cell the one that starts on the earlier edge in the order B, R, T, L comes first.
 *   Output order: cells in ascending iy*(nx-1)+ix, within a cell as above.  *count is the total number of segments.  A segment whose
 *     index is >= cap_segments is not written and memory behind the capacity is never touched; the call returns SPHX_OK either way (the
 *     caller compares count with its capacity).  segments NULL: the count alone.  Two calls on one state return the same bytes: no atomic
 *     decides an order.
 *   When allowed, refusals, side effects: as sphx_sample_grid (the same SPHX_ERR_NOT_READY rules and lattice errors, a tile context is
 *     refused, the call only reads).  Further argument errors: iso not finite, unknown field, unknown flag bit, out or out->count NULL.
 *     nx < 2, ny < 2 or nx*ny == 0 is a successful call with count = 0; values is still filled when nx*ny > 0.
 * SPHX_CONTOUR_DEVICE_POINTERS: every pointer of out is a device pointer; the call is enqueued on the context's stream and returns
 * without waiting, and nothing crosses to the host between the sampling and the segments.  Without it: host pointers, the call returns
 * when they are written (through a device scratch grown on demand and freed in sphx_destroy).
 * sphx_contour_chain (pure host code, no context): segment u follows s when start(u) == end(s) — fp32 == on both coordinates, so NaN
 *   equals nothing and -0 equals +0.  successor(s) is the lowest-index unused such u.  Pass 1: in ascending index, every unused segment
 *   whose start equals no segment's end opens a line, which follows successors until there is none (an open line).  Pass 2: in ascending
 *   index, every segment still unused opens a line that follows successors; it is closed iff the end of its last segment equals the
 *   start of its first.  order[n] lists the segment indices line after line, line_first[k] is the first position of line k in order and
 *   line_first[lines] = n, closed[k] is 0 or 1, *out_lines the number of lines.  O(n log n).  n == 0 succeeds with *out_lines = 0 (the
 *   pointers but out_lines may be NULL); a NULL pointer with n > 0 (or out_lines NULL) returns SPHX_ERR_INVALID_ARGUMENT. */
enum { SPHX_CONTOUR_FIELD_FRACTION = 0, SPHX_CONTOUR_FIELD_DENSITY = 1 };
enum { SPHX_CONTOUR_DEVICE_POINTERS = 1u };   /* as SPHX_SAMPLE_DEVICE_POINTERS: enqueued on the context's stream, no wait */
typedef struct sphx_contour_out {
    float*    segments;  /* [cap_segments][4] = x0, y0, x1, y1, or NULL (count only) */
    uint32_t* cell;      /* [cap_segments] cell index iy*(nx-1)+ix of each segment, or NULL */
    float*    values;    /* [nx*ny] the lattice values the contour was cut from, or NULL */
    uint32_t* count;     /* [1] total number of segments; required */
} sphx_contour_out;
int sphx_surface_contour(sphx_ctx* ctx, float x0, float y0, float dx, float dy, uint32_t nx, uint32_t ny, int kernel_kind,
                         int field, float iso, uint32_t cap_segments, uint32_t flags, const sphx_contour_out* out);
int sphx_contour_chain(const float* segments, uint32_t n, uint32_t* order /* [n] */, uint32_t* line_first /* [n+1] */,
                       uint8_t* closed /* [n] */, uint32_t* out_lines);

/* ---- rendering: the reference app's picture of the particles (main.rs:239-275 draw_fluid, recording mode :310-331, :380-397) ---------
 * Every fluid particle a disc coloured heatmap_color(|v| * speed_scale), drawn in array order over the grey boundary particles over the
 * background, through the Camera of camera.rs — as an RGBA8 image and / or an image of owners, on the device: a frame is 4 bytes per pixel
 * instead of 12 per particle (sphx_view_*).  The contract, for pixel (ix, iy) of a view, all in fp32 and unfused:
 *   inv = 1.0f / pixel_per_world_unit;
 *   qx = center[0] + (((float)ix + 0.5f) - 0.5f * (float)width) * inv,
 *   qy = center[1] - (((float)iy + 0.5f) - 0.5f * (float)height) * inv      (the inverse of Camera::world_to_screen_coords, camera.rs:43-51,
 *                                                                             at the pixel centre; row 0 is the TOP row)
 *   r = max(radius != 0 ? radius : particle_radius, min_pixel_radius * inv), r2 = r * r.
 *   Particle j COVERS the pixel iff dx = x_j.x - qx, dy = x_j.y - qy, d2 = dx*dx + dy*dy, d2 <= r2.  A non-finite position covers nothing.
 *   owner = the highest device index j (the order of sphx_download) among ALL fluid particles that cover the pixel — the reference draws
 *           its instances in array order, later over earlier (main.rs:242-258); else SPHX_RENDER_BOUNDARY if any boundary particle covers
 *           it (boundary instances come first, main.rs:160-170); else SPHX_RENDER_NONE.  Not a cell neighbourhood: all particles.
 *   rgba  = the background / boundary bytes as given; for a fluid owner j with velocity v (sphx_download's): s = sqrtf(v.x*v.x + v.y*v.y)
 *           (correctly rounded), t = s * speed_scale, c_k = t * 3.0f - (float)k for k = 0, 1, 2 (heatmap_color, main.rs:74-80) clamped to
 *           [0, 1] with a NaN becoming 0, byte (uint8_t)(c_k * 255.0f + 0.5f), alpha 255.
 * The result is a pure function of the downloaded arrays and the view.  Deviations from the reference's GPU pipeline: an exact disc
 * instead of Mesh::new_circle's polygon (tolerance 0.0003, main.rs:104-112), pixel-centre coverage without multisampling, no sRGB
 * conversion (parity unpinned: ggez is not in the tree).
 * min_pixel_radius makes a zoomed-out frame useful: every point of the image is within sqrt(0.5) ~ 0.7071 pixels of a pixel centre, so with
 * min_pixel_radius >= 0.7072 every particle inside the image covers at least one pixel.
 * When the call is allowed: wherever sphx_download is (after an upload, after a finished step of either solver; a pending advection is
 * applied first, as there); it needs no neighbour build and no densities.  Between a step_begin and its step_finish: SPHX_ERR_NOT_READY.
 * Before any upload (N = 0): the boundary over the background.  A tile context (sphx_tile_*, sphx_multi_tile_ctx) is refused with
 * SPHX_ERR_INVALID_ARGUMENT (it holds ghosts; a tiled run is drawn by sphx_multi_render, "picture of a tiled run" below).  N <= 2^32 - 3
 * (two owner codes are taken).
 * Argument errors (SPHX_ERR_INVALID_ARGUMENT, the message names the argument): view / out NULL, both outputs NULL, unknown flag bits,
 * pixel_per_world_unit / center / radius / min_pixel_radius / speed_scale not finite, pixel_per_world_unit <= 0, radius < 0 or
 * > smoothing_length, min_pixel_radius < 0 or > 4, width * height >= 2^28.  width * height == 0 is a successful no-op.  The two upper
 * bounds keep a call's work bounded whatever the view: a disc of radius h is overdrawn ~13 times at rest density, a disc of 4 pixels
 * touches at most 81 pixels per particle.
 * No side effects: like a sampling query the call only reads; a run with renders between its steps is bit-identical to one without. */
typedef struct sphx_render_view {
    uint32_t width, height;      /* pixels; row 0 is the TOP row (screen coordinates, camera.rs:43-51) */
    float center[2];             /* Camera::position: the world point in the middle of the image */
    float pixel_per_world_unit;  /* Camera::pixel_per_world_unit (finite, > 0) */
    float radius;                /* disc radius in world units, <= smoothing_length; 0 = particle_radius (main.rs:103-108) */
    float min_pixel_radius;      /* lower bound of the disc radius, in pixels, <= 4; 0 = none (the reference) */
    float speed_scale;           /* heat-map argument t = |v| * speed_scale; main.rs:255 uses 0.1 */
    uint8_t background[4];       /* main.rs:369: (0.4, 0.4, 0.45, 1) -> 102, 102, 115, 255 */
    uint8_t boundary[4];         /* main.rs:153-158: 0.2 grey -> 51, 51, 51, 255 */
    uint32_t reserved[2];
} sphx_render_view;              /* 48 bytes */
typedef struct sphx_render_out {
    uint8_t* rgba;    /* [height*width*4], bytes r, g, b, a, or NULL (a device pointer must be 4-byte aligned) */
    uint32_t* owner;  /* [height*width] or NULL */
} sphx_render_out;
enum { SPHX_RENDER_NONE = 0xFFFFFFFFu, SPHX_RENDER_BOUNDARY = 0xFFFFFFFEu };
enum { SPHX_RENDER_DEVICE_POINTERS = 1u }; /* as SPHX_SAMPLE_DEVICE_POINTERS: the outputs are device pointers, the call is enqueued on the
                                              context's stream and does not wait */
/* Camera::center_around_world_rect (camera.rs:21-35) for the screen (0, 0, width, height) and the world rectangle (x, y, w, h):
 * pixel_per_world_unit = min(width / w, height / h), center = (x + w * 0.5, y + h * 0.5); plus the app's defaults (radius 0,
 * min_pixel_radius 0, speed_scale 0.1, the two colours above).  Pure host code, needs no context and no GPU.  SPHX_ERR_INVALID_ARGUMENT
 * for out NULL, a non-finite number, or w / h <= 0. */
int sphx_render_fit(uint32_t width, uint32_t height, float x, float y, float w, float h, sphx_render_view* out);
int sphx_render(sphx_ctx* ctx, const sphx_render_view* view, uint32_t flags, const sphx_render_out* out);

/* ---- emitting and draining fluid: the particle set edited on the device (an inflow, an outflow, a keep-box) -----------------------------
 * The reference can only add (a caller pushes onto the world's Vecs; dfsph.rs:418 "removing this way is impossible with this design") and
 * carries a stop-gap for "endlessly falling particles" (main.rs:189-192).  Both calls edit the cell-ordered device arrays in place of the
 * round trip sphx_download, filter / concatenate on the host, sphx_upload.  The contract:
 *   Predicate (sphx_remove), in fp32 with IEEE comparisons — a NaN coordinate is in no rectangle:
 *     in(r, p) = p.x >= r.x0 && p.x < r.x1 && p.y >= r.y0 && p.y < r.y1;  hit = in(r, p) for any of the n_rects rectangles.
 *     A particle is removed iff hit — with SPHX_REMOVE_OUTSIDE iff !hit: the rectangles are then a keep-box, and NaN particles go.
 *     +-inf bounds are allowed (half planes); x0 > x1 or y0 > y1 is an empty rectangle.  n_rects == 0 removes nothing, or everything with
 *     SPHX_REMOVE_OUTSIDE.  A NaN bound, n_rects > SPHX_REMOVE_MAX_RECTS, rects NULL with n_rects > 0 or unknown flag bits:
 *     SPHX_ERR_INVALID_ARGUMENT.
 *   Remove: the survivors keep their relative (cell-sorted) order; position, velocity and particle_id travel with the particle.  alpha,
 *     kappa, stiffness, the WCSPH accelerations and density[] are bound to their SLOT and are not moved — what the reference's Vec::resize
 *     truncation (dfsph.rs:420-422, wscsph.rs:129) and the round trip leave behind.  The density sphx_download returns is unspecified until
 *     the next step or sphx_update_densities.  N becomes the survivor count (0 is legal); *out_removed (may be NULL) the number removed.
 *   Append: the m records go to [N, N + m) (vel_xy NULL = zero velocities), with particle_id first_id + k, where first_id = *out_first_id
 *     (may be NULL) = the number of particles uploaded or appended since the last sphx_upload.  Ids are never reused (removing does not
 *     free any); running past 2^32 returns SPHX_ERR_CAPACITY.  sphx_upload keeps its meaning (ids 0 .. n - 1) and resets the counter to n.
 *     When N + m exceeds the allocated capacity the arrays grow by half (at least to N + m) and the present particles are copied on the
 *     device; sphx_reserve before the upload avoids that.
 *   Solver caches: both calls leave the cached array length (dfsph.rs:419) alone and mark the particle set as changed; the next
 *     sphx_step_begin[_law] then runs the warm-up block (dfsph.rs:419-428, SPHX_FLAG_WARMUP) even when the count has come back to the cached
 *     length (remove k, append k) — the one deliberate difference from the round trip, which would walk the lists of another set there.
 *     The iteration counts (warm starts) are kept, the WCSPH accelerations as after sphx_upload of the same count.
 *   Equivalence: apart from the ids and that corner, the state after sphx_append is the state download, concatenate, sphx_upload leaves
 *     in a context with the same history, the state after sphx_remove the state download, filter, sphx_upload leaves; every later step
 *     is bit-identical to that context's.
 *   Nothing removed (or m == 0): the context is untouched — lists, sampling state and a queued run-ahead pass stay valid.
 *   Something removed or appended: the neighbour lists and the sampling state are stale (sphx_sample_* returns SPHX_ERR_NOT_READY until a
 *     step or sphx_update_neighborhood + sphx_update_densities); sphx_render and sphx_download work at once on the new set.
 *   Refusals: SPHX_ERR_NOT_READY between a step_begin and its step_finish (either solver) and before the first sphx_upload (an upload of
 *     zero particles counts); SPHX_ERR_INVALID_ARGUMENT on a tile context (sphx_tile_*, sphx_multi_tile_ctx: it holds ghosts) and in
 *     tiling-invariant mode (sphx_set_tiling_invariant).  A tiled run is edited through sphx_multi_append / sphx_multi_remove ("emitting
 *     and draining fluid in a tiled run" below), which work in either mode.
 * Cost: sphx_remove reads 8 bytes per particle for the predicate and moves 40 bytes per survivor only when something goes; one 4-byte
 * count comes back to the host (the call's only synchronisation).  sphx_append copies the new records and nothing else while they fit. */
typedef struct sphx_rect { float x0, y0, x1, y1; } sphx_rect; /* [x0, x1) x [y0, y1) in world units */
#define SPHX_REMOVE_MAX_RECTS 8
enum { SPHX_REMOVE_OUTSIDE = 1u }; /* remove what is in NO rectangle */
int sphx_append(sphx_ctx* ctx, const float* pos_xy, const float* vel_xy /* NULL = 0 */, uint32_t m, uint32_t* out_first_id /* may be NULL */);
int sphx_remove(sphx_ctx* ctx, const sphx_rect* rects, uint32_t n_rects, uint32_t flags, uint32_t* out_removed /* may be NULL */);

/* ---- neighbour queries: which particles lie around given points, which lie in given rectangles (neighborhood_search.rs as a service) ----
 * sphx_sample_points walks the candidates of a point and returns sums; sphx_remove evaluates a region and deletes.  These two calls
 * return the IDENTITIES instead — a viewer picks the particle under the cursor and follows it (sphx_track_set), a coupling code gathers
 * the fluid around its own points, a region is tagged — without sphx_download and a grid rebuilt on the host.
 * sphx_query_radius, for a query point q (fp32 x, y), all in fp32 and unfused:
 *   Candidates: those of sphx_sample_points — with (cx, cy) the cell of q, computed as for a particle, the particles of the 3x3 cells
 *     around (cx, cy) in ascending device index.  Without SPHX_QUERY_BOUNDARY the fluid particles (the order of sphx_download), with it
 *     the boundary particles (the order of sphx_download_boundary): one call answers over ONE set.  A stray particle, which the grid
 *     holds no cell for (SPHX_FLAG_STRAY_PARTICLES), is never a candidate.
 *   Acceptance: dx = x_j.x - q.x, dy = x_j.y - q.y, d2 = dx*dx + dy*dy; accepted iff d2 <= r2, r2 = radius * radius.  There is no
 *     d2 > 1e-10 exclusion: a point on a particle finds it at d2 = 0.  dist_sq holds the bits of d2.
 *   Entries: the entries of a point are its accepted candidates in candidate order; the points follow each other in the caller's order
 *     (CSR: point k owns [offsets[k], offsets[k+1]), offsets[m] = *count = the total).
 *   Nearest: the accepted candidate with the smallest d2 — compared with fp32 < in candidate order, so a tie goes to the lowest index;
 *     SPHX_QUERY_NONE and the word 0x7F800000 (+inf) where nothing is accepted.
 *   Bad points: a NaN point or one far outside the domain gets no entry (a NaN coordinate saturates to cell 0 and fails every distance
 *     test); it never faults.
 *   THE BOX RULE IS THE CONTRACT, not "all particles within radius": the cell size is h = smoothing_length, and a particle exactly h
 *     away can sit two cells off after the rounding of the cell function (on the 4 050-particle dam break and the 22 000 points of
 *     tests/test_query_host.py, radius == h misses 78 of 20 167 boundary pairs and no fluid pair that a search over all particles
 *     accepts; the neighbour build behaves alike).  For radius <= 0.9 * smoothing_length the result is the set a search over all
 *     particles finds (there: exact agreement at 0.9 h and 0.5 h, both sets).
 *   Radius: finite, > 0 and <= smoothing_length, else SPHX_ERR_INVALID_ARGUMENT.  r2 may underflow to 0: then only d2 == 0 is accepted.
 *   Capacity: an entry at position >= cap_entries is not written and memory behind the capacity is never touched; the call returns
 *     SPHX_OK either way; offsets and count always describe the FULL result.  With index, id and dist_sq all NULL the call walks once
 *     and writes nothing per entry.
 *   Determinism: no atomic decides a position; two calls on one state return the same bytes.
 *   When allowed, refusals, side effects: as sphx_sample_points (the same SPHX_ERR_NOT_READY rules; the call only reads, a run with
 *     queries between its steps is bit-identical to one without).  A tile context is refused with SPHX_ERR_INVALID_ARGUMENT; a tiled
 *     run is served by sphx_multi_query_radius and sphx_multi_select ("neighbour queries of a tiled run").  m == 0 succeeds with *count = 0 (and offsets[0] = 0 when offsets is given).
 *   Argument errors (SPHX_ERR_INVALID_ARGUMENT, the message names the argument): out or out->count NULL, xy NULL with m > 0, unknown
 *     flag bits, m >= 2^31, a bad radius, a device offsets or count pointer that is not 8-byte aligned.
 * SPHX_QUERY_DEVICE_POINTERS: xy and every pointer of out are device pointers; everything is enqueued on the context's stream without
 *   a wait and nothing crosses to the host.  Without it: host pointers; the call goes through a device scratch grown on demand and freed
 *   in sphx_destroy, reads the total once and copies min(total, cap_entries) entries.
 * Points are processed in the caller's order, one lane each: pass large point sets SPATIALLY COHERENT, as for sphx_sample_points.
 * Cost: one walk for the counts, offsets and nearest; a second walk plus 12 bytes per entry for the lists.
 *
 * sphx_select: the predicate of sphx_remove, bit for bit (the same rectangles, NaN rules, infinite bounds, empty rectangles and
 *   SPHX_REMOVE_MAX_RECTS; SPHX_SELECT_OUTSIDE as SPHX_REMOVE_OUTSIDE) — and nothing is removed: the particles that sphx_remove would
 *   remove come out in ascending device index as index[] (the order of sphx_download) and id[] (particle_id); *count is their number,
 *   the capacity rule is that of the query.  Allowed wherever sphx_download is (a pending advection is applied first, as in sphx_render);
 *   SPHX_ERR_NOT_READY between a step_begin and its step_finish; a tile context is refused.  It only reads.  A stable compaction on the
 *   device without atomics.  Argument errors: sphx_remove's, and out or out->count NULL. */
typedef struct sphx_query_out {
    uint64_t* offsets;          /* [m+1] CSR: entries of point k are [offsets[k], offsets[k+1]); offsets[m] = total.  or NULL */
    uint32_t* index;            /* [cap_entries] device index (order of sphx_download; with SPHX_QUERY_BOUNDARY: of sphx_download_boundary), or NULL */
    uint32_t* id;               /* [cap_entries] particle_id (with SPHX_QUERY_BOUNDARY: boundary_id), or NULL */
    float*    dist_sq;          /* [cap_entries] the d2 of the acceptance test, or NULL */
    uint32_t* nearest;          /* [m] index of the nearest accepted candidate, SPHX_QUERY_NONE if none, or NULL */
    float*    nearest_dist_sq;  /* [m] its d2; the word 0x7F800000 (+inf) if none, or NULL */
    uint64_t* count;            /* [1] total entries; required */
} sphx_query_out;               /* 56 bytes */
enum { SPHX_QUERY_DEVICE_POINTERS = 1u, SPHX_QUERY_BOUNDARY = 2u };
#define SPHX_QUERY_NONE 0xFFFFFFFFu
int sphx_query_radius(sphx_ctx* ctx, const float* xy, uint32_t m, float radius, uint64_t cap_entries, uint32_t flags, const sphx_query_out* out);
typedef struct sphx_select_out {
    uint32_t* index;  /* [cap] device index, or NULL */
    uint32_t* id;     /* [cap] particle_id, or NULL */
    uint32_t* count;  /* [1] number selected; required */
} sphx_select_out;    /* 24 bytes */
enum { SPHX_SELECT_OUTSIDE = 1u, SPHX_SELECT_DEVICE_POINTERS = 2u };
int sphx_select(sphx_ctx* ctx, const sphx_rect* rects, uint32_t n_rects, uint32_t flags, uint32_t cap, const sphx_select_out* out);

/* ---- saving and restoring a context: a run that can be put down and picked up (restart files, roll-back, late-window measurements) --------
 * sphx_state_save writes everything a later step of this context can read into one self-describing blob; sphx_state_load puts it back, into
 * this context, a fresh one or one in another process.  The promise: a context that loads a blob and then receives the calls the saving
 * context received after the save produces the same bits — every sphx_step_stats field, every array and neighbour list, every sample and
 * render — as long as neither run raises SPHX_FLAG_STRAY_PARTICLES or SPHX_FLAG_DENSE_CELL (the covered region is derived again at load;
 * the order inside a dense cell was never deterministic).  Save only reads: a run with saves between its steps is bit-identical to one
 * without (a queued run-ahead pass stays valid).
 * The blob (little-endian; the byte-exact layout is the comment at the top of csrc/sphx_state_format.hpp, which also holds its validation
 * as plain host C++): a fixed header — magic, format version, endianness tag, total size —, the sphx_params of the context (device stored
 * as 0), the scalars N, B, cached_n (dfsph.rs:419), wcsph_n, ids_issued (sphx_append), the two iteration counts behind the warm starts
 * (dfsph.rs:199 / :354), and the flags "particle set changed" (sphx_append / sphx_remove), tiling-invariant mode, "the neighbour lists belong
 * to the positions" and "sampling allowed"; a table of {offset, bytes, digest} per section and a digest of the header itself; then the SPHX_STATE_SECTIONS sections, 8-byte
 * aligned, padding zero: positions, velocities and particle_id of the N particles in device order (sphx_download), density[N], the slot-bound
 * alpha, kappa and stiffness for the first min(N, cached_n) slots (sphx_download_solver_state), the WCSPH accelerations accel[wcsph_n], and
 * the boundary in CALLER order (as given to sphx_set_boundary).  No timestamp, no pointer, no capacity: two saves of one state are
 * byte-identical.  Neighbour lists, cell grids, the covered region and scratch are not stored: they are functions of what is.
 * Section digest: the section as W 32-bit words w[0 .. W), all arithmetic mod 2^64 with a 64-bit word index i:
 *     digest = sum_i (uint64)w[i] * ((2 i + 1) * 0x9E3779B97F4A7C15)  +  W * 0xD6E8FEB86659FD93
 *   position-weighted (swapped words change it) and independent of the order of accumulation, so the device computes it in one streaming
 *   pass and the host reproduces it exactly.  An INTEGRITY CHECK and a fingerprint — NOT a cryptographic hash: it detects damage and lets
 *   two runs be compared by 8 bytes per array, it does not resist someone who wants a collision.
 *   sphx_state_digest: the digests of the LIVE state, out[SPHX_STATE_SEC_*] (72 bytes come back; nothing else is downloaded).  Save stores
 *   the same numbers in the table; load recomputes them on the device after the copy and compares.
 * Load validates on the host first — magic, version, endianness, sizes, section bounds and overlaps, every count against every other, and
 *   the params: every field except device and list_span_limit must equal this context's bit for bit (the message names the first that does
 *   not); a blob saved in tiling-invariant mode loads only into a context in that mode and the other way round.  A refusal at this stage is
 *   SPHX_ERR_INVALID_ARGUMENT and leaves the context UNTOUCHED.  Then load allocates as sphx_upload does (an earlier sphx_reserve holds),
 *   installs the boundary and the arrays in the saved order, zero-fills the slot-bound slots the blob does not hold, sets the scalars and
 *   drops a queued run-ahead pass.  If the lists were current at save it runs ONE neighbour build — not a step: it raises no flag and
 *   computes neither density nor alpha, and since a re-grid of an already sorted set is the identity the arrays stay as loaded — so that the
 *   next sphx_step_begin finds what the saving context had; if sampling was allowed at save it is allowed after load.  A digest that does
 *   not match after the copy: SPHX_ERR_INVALID_ARGUMENT naming the section; the context then asks for an upload or a load (every step call
 *   returns SPHX_ERR_NOT_READY), as after a failed step.  A malformed blob never faults: no count is used before it has been checked.
 *   One deliberate difference: a blob whose lists were NOT current although the next step would have walked them (sphx_upload of the cached
 *   count without sphx_clear_cached: the reference walks stale lists there, dfsph.rs:419) loads with the "set changed" mark, i.e. the next
 *   step runs the warm-up block — stale lists are not state anybody can restore.
 * SPHX_STATE_DEVICE_BUFFER: buf is device memory on the context's device; the sections are copied device-to-device (the header, the
 *   positions and the boundary also cross to the host: the 392-byte header on save; on load the host derives the covered region from the positions
 *   and keeps the boundary's caller order).  The call returns when buf is complete (save) or no longer needed (load).
 * When allowed: save wherever sphx_download is; save and digest return SPHX_ERR_NOT_READY before the first upload or load and after a
 *   failed step; save, load and digest return SPHX_ERR_NOT_READY between a step_begin and its step_finish (either solver); load is allowed
 *   on any context outside a step.  A tile context (sphx_tile_*, sphx_multi_tile_ctx): SPHX_ERR_INVALID_ARGUMENT.  A capacity smaller than
 *   sphx_state_size: SPHX_ERR_CAPACITY with the needed size in *out_bytes (out_bytes may be NULL).  sphx_multi_* has NO counterpart yet: a
 *   multi-GPU run cannot be saved (sphx_solver_save on the multi-GPU solver object: SPHX_ERR_INVALID_ARGUMENT).  (That holds for THESE
 *   calls and this blob; a tiled run has a checkpoint of its own: sphx_multi_state_*, "checkpoint of a tiled run" below.)
 * Files: sphx_state_save_file writes exactly the blob (to path + ".tmp", renamed when complete), sphx_state_load_file reads one; an I/O
 *   failure is SPHX_ERR_INVALID_ARGUMENT with errno's text. */
#define SPHX_STATE_SECTIONS 9
enum {
    SPHX_STATE_SEC_POSITIONS = 0, SPHX_STATE_SEC_VELOCITIES = 1, SPHX_STATE_SEC_PARTICLE_ID = 2, SPHX_STATE_SEC_DENSITY = 3, SPHX_STATE_SEC_ALPHA = 4,
    SPHX_STATE_SEC_KAPPA = 5, SPHX_STATE_SEC_STIFFNESS = 6, SPHX_STATE_SEC_ACCEL = 7, SPHX_STATE_SEC_BOUNDARY = 8
};
enum { SPHX_STATE_DEVICE_BUFFER = 1u };
int sphx_state_size(sphx_ctx* ctx, uint64_t* out_bytes);
int sphx_state_save(sphx_ctx* ctx, void* buf, uint64_t capacity, uint32_t flags, uint64_t* out_bytes /* may be NULL */);
int sphx_state_load(sphx_ctx* ctx, const void* buf, uint64_t bytes, uint32_t flags);
int sphx_state_digest(sphx_ctx* ctx, uint64_t* out /* [SPHX_STATE_SECTIONS] */);
int sphx_state_save_file(sphx_ctx* ctx, const char* path);
int sphx_state_load_file(sphx_ctx* ctx, const char* path);

/* ---- following particles by id: look-up, id-ordered download, trajectories (csrc/sphx_track.inc) -----------------------------------------
 * The device re-sorts its particles on every step; particle_id[] travels with them.  These calls answer "where is particle id now" on the
 * device — 4 bytes per particle scanned — instead of a full sphx_download and an argsort on the host.  (sphx_view_* cannot stand in: it
 * packs every stride-th SLOT, and a slot holds another particle after each re-grid.)
 * Slot of an id: slot_of(id) = the HIGHEST device index j < N with particle_id[j] == id, or SPHX_TRACK_ABSENT if there is none; "device
 *   index" is the order of sphx_download.  Ids are unique in a context filled by sphx_upload / sphx_append; a context that loaded a blob
 *   with repeated ids (sphx_state_load does not refuse one) gets the same answer on every call (an integer maximum of slot + 1, no race).
 * Fetch: sphx_track_set hands over m ids (host memory, copied; any order, duplicates allowed and answered alike; m == 0 clears the set).
 *   sphx_track_fetch then gives, for the k-th id in the caller's order: slot[k] = slot_of(ids[k]); pos, vel and density = the exact bits
 *   sphx_download returns at that slot.  For an absent id every float is the word 0x7FC00000 and the slot is SPHX_TRACK_ABSENT.  An empty
 *   set is a successful no-op.
 * sphx_download_by_id: the same rule for the ids first_id + k, k < count; *out_present = the number of ids found.  first_id + count may
 *   reach 2^32 and no more (SPHX_ERR_INVALID_ARGUMENT beyond); count == 0 is a successful no-op (*out_present = 0).  With first_id = 0 and
 *   count = n after an unedited sphx_upload of n particles the result is the particles in upload order, whatever the steps since.
 * SPHX_TRACK_DEVICE_POINTERS (fetch, read, download_by_id): every output — out_present too — is a device pointer on the context's device;
 *   the call is enqueued on the context's stream and returns without waiting.  Without it: host pointers; the call returns when they are
 *   written (through a device scratch the library grows on demand and frees in sphx_destroy).
 * Recording: after sphx_track_record(max_frames, every) every every-th SUCCESSFULLY finished step (either solver, counted from the call;
 *   so also each step inside sphx_solver_simulation_steps) enqueues one frame behind its own kernels: {x, y, vx, vy} per tracked id in the
 *   caller's order, 16 bytes each, four 0x7FC00000 words for an absent id.  Nothing comes back to the host and nothing is synchronised.
 *   A failed step takes no frame and does not count.  Once max_frames frames are stored, later frames are counted in `dropped` and not
 *   stored.  The buffer is max_frames * m * 16 bytes on the device; more than 1 GiB is SPHX_ERR_CAPACITY.  sphx_track_read copies the
 *   frames [first_frame, first_frame + n_frames) to out[n_frames][m][4]; a range beyond `frames` is SPHX_ERR_INVALID_ARGUMENT; the host
 *   path waits for the stream.  sphx_track_set and sphx_track_record discard an earlier recording; max_frames == 0 stops and frees;
 *   every == 0 is SPHX_ERR_INVALID_ARGUMENT; recording with an empty set is SPHX_ERR_NOT_READY.
 * Lifetime: the set and the recording belong to the CONTEXT, not to the particle state.  sphx_append / sphx_remove leave them alone (a
 *   removed id becomes absent, an appended id that is in the set is found).  sphx_upload renumbers the particles: the set keeps its numbers
 *   and now means the new particles.  sphx_state_save does not store them; sphx_state_load leaves them as they are.
 * No side effects: all of this only reads the particle state.  A run with a tracked set, fetches, by-id downloads and a recording is
 *   bit-identical to the same run without them — every sphx_state_digest word, every sphx_step_stats field, sphx_last_flags — and a queued
 *   run-ahead pass stays valid, as for sphx_sample_*.
 * When allowed: fetch and sphx_download_by_id wherever sphx_download is, and before any upload (N = 0: everything is absent).  Fetch, read,
 *   sphx_download_by_id, set and record return SPHX_ERR_NOT_READY between a step_begin and its step_finish (either solver).  A tile context
 *   (sphx_tile_*, sphx_multi_tile_ctx) is refused with SPHX_ERR_INVALID_ARGUMENT: it holds ghosts and its ids need not be unique.
 *   sphx_multi_* has NO counterpart that takes a sphx_ctx: THESE calls never serve a tile.  A tiled run is followed through calls of its
 *   own, sphx_multi_track_* and sphx_multi_download_by_id ("following particles by id in a tiled run" below), not through sphx_multi_download.
 * Argument errors (SPHX_ERR_INVALID_ARGUMENT, the message names the argument): ctx, out or status NULL, every output NULL, ids NULL with
 *   m > 0, m > SPHX_TRACK_MAX_IDS, unknown flag bits.
 * Cost: the look-up streams particle_id[] once (4 bytes per particle; a bit filter in LDS keeps all but ~6 % of the other particles away
 *   from the binary search of the sorted id table), then 28 bytes per id found; a frame entry is 16 bytes ("Following particles"). */
#define SPHX_TRACK_MAX_IDS 16384
#define SPHX_TRACK_ABSENT  0xFFFFFFFFu
enum { SPHX_TRACK_DEVICE_POINTERS = 1u };
typedef struct sphx_track_out {
    uint32_t* slot;   /* [m] or NULL */
    float* pos;       /* [2m] interleaved xy, or NULL */
    float* vel;       /* [2m] interleaved xy, or NULL */
    float* density;   /* [m] or NULL */
} sphx_track_out;     /* not all NULL */
typedef struct sphx_track_status { uint32_t m, recording, max_frames, every, frames, dropped, reserved[2]; } sphx_track_status;
int sphx_track_set(sphx_ctx* ctx, const uint32_t* ids /* host */, uint32_t m);
int sphx_track_fetch(sphx_ctx* ctx, uint32_t flags, const sphx_track_out* out);
int sphx_track_record(sphx_ctx* ctx, uint32_t max_frames, uint32_t every);
int sphx_track_get_status(const sphx_ctx* ctx, sphx_track_status* out);
int sphx_track_read(sphx_ctx* ctx, uint32_t first_frame, uint32_t n_frames, uint32_t flags, float* out /* [n_frames][m][4] = x, y, vx, vy */);
int sphx_download_by_id(sphx_ctx* ctx, uint32_t first_id, uint32_t count, uint32_t flags, const sphx_track_out* out, uint32_t* out_present /* may be NULL */);

/* ---- per-particle flow fields: velocity gradient, divergence, vorticity and the colour-field gradient (csrc/sphx_fields.inc) ---------------
 * What people derive from an SPH velocity field AT THE PARTICLES — vortex visualisation, what the divergence solver left behind, free-surface
 * detection and surface normals — from one more traversal of the solver's own neighbour lists, run on request: 32 bytes per particle come
 * out instead of sphx_download + sphx_download_neighbors and a host loop.  (sphx_sample_* cannot stand in: it interpolates at query points
 * from cell scans and knows nothing of differences v_j - v_i over the solver's neighbour set.)
 * The contract, for particle i (device order: the order of sphx_download, n = sphx_num_particles): walk the entries 0 .. count_total - 1 of
 *   its neighbour list in list order — dynamic entries first, then static ones: exactly what sphx_download_neighbors returns; a list the
 *   build capped at 64 entries (SPHX_FLAG_NEIGHBOR_CAP) stays capped, the fields see what the solver sees.  All arithmetic fp32 and unfused,
 *   every sum starts at 0.0f and takes one rounding per operation:
 *     dx = x_j.x - x_i.x, dy = x_j.y - x_i.y, d2 = dx*dx + dy*dy, r = sqrtf(d2) (correctly rounded), q = min(r * w_hinv, 1), omq = 1 - q,
 *     s = ((w_ngrad*omq)*omq)*omq, gx = s*dx, gy = s*dy       (Kernel::gradient_from_positions(x_i, x_j), kernel.rs:23-28 with
 *                                                              wendland_quintic_c2.rs:42-46; w_hinv, w_ngrad = sphx_get_constants out[0], out[2])
 *     vol = m / rho_j for a fluid neighbour (rho_j = the density sphx_download returns), vol = m / rho0 and v_j = (0, 0) for a boundary one
 *     ax = vol*gx, ay = vol*gy, dvx = v_j.x - v_i.x, dvy = v_j.y - v_i.y          (v = sphx_download's velocity)
 *     Lxx = Lxx + dvx*ax, Lxy = Lxy + dvx*ay, Lyx = Lyx + dvy*ax, Lyy = Lyy + dvy*ay, cx = cx + ax, cy = cy + ay
 *   and after the walk  vel_grad = {Lxx, Lxy, Lyx, Lyy} (d(vx)/dx, d(vx)/dy, d(vy)/dx, d(vy)/dy), divergence = Lxx + Lyy,
 *   vorticity = Lyx - Lxy, color_grad = {cx, cy}.  color_grad is the gradient of the colour field: ~0 in the bulk and next to a wall, pointing
 *   INTO the fluid at a free surface (|color_grad| * h of order 1 there; no threshold is built in).  A particle with an empty list gets zeros.
 *   Any subset of the outputs gives the same bits as the full set.
 * When the call is allowed: as for sphx_sample_* — the neighbour lists and density[] must belong to the current positions: after a finished
 *   step of either solver that ran a neighbour build (not one over zero fluid particles), after sphx_update_neighborhood followed by
 *   sphx_update_densities, and after a sphx_state_load of such a state.  After sphx_upload, sphx_set_boundary, sphx_append / sphx_remove (that
 *   changed something), between a step_begin and its step_finish and after a failed step: SPHX_ERR_NOT_READY, with the messages of sampling.
 *   A tile context (sphx_tile_*, sphx_multi_tile_ctx) is refused with SPHX_ERR_INVALID_ARGUMENT; a tiled run is served by
 *   sphx_multi_particle_fields ("per-particle flow fields of a tiled run", below).
 * Argument errors (SPHX_ERR_INVALID_ARGUMENT, the message names the argument): ctx or out NULL, every output NULL, unknown flag bits.
 *   n == 0 in a ready context is a successful no-op.
 * No side effects: the call only reads (it restores the sweep direction a launch toggles and leaves a queued run-ahead pass valid); a run
 *   with calls between its steps is bit-identical to one without — every sphx_state_digest word, every sphx_step_stats field, sphx_last_flags.
 * SPHX_FIELDS_DEVICE_POINTERS: the outputs are device pointers on the context's device (4-byte alignment suffices); the call is enqueued
 *   on the context's stream and does not wait.
 *   Without it: host pointers; the call goes through a device scratch the library grows on demand for the requested outputs only and frees
 *   in sphx_destroy, and returns when the outputs are written.
 * Cost: the staged record of the non-pressure pass (position, velocity, one scalar), walked over count_total entries; DESIGN.md section 4h. */
typedef struct sphx_fields_out {
    float* vel_grad;    /* [4n]: d(vx)/dx, d(vx)/dy, d(vy)/dx, d(vy)/dy per particle, or NULL */
    float* divergence;  /* [n] or NULL */
    float* vorticity;   /* [n] or NULL */
    float* color_grad;  /* [2n] interleaved xy, or NULL */
} sphx_fields_out;      /* not all NULL */
enum { SPHX_FIELDS_DEVICE_POINTERS = 1u };
int sphx_particle_fields(sphx_ctx* ctx, uint32_t flags, const sphx_fields_out* out);

/* ---- fluid statistics: counts, sums, extremes, probe rectangles, time series (csrc/sphx_stats.inc) -----------------------------------------
 * What an SPH user checks first — is the run healthy: total momentum and kinetic energy, where the fluid is (bounds, centre of mass), how
 * compressed it is (density spread), whether anything has gone non-finite — from one streaming pass on the device, 20 bytes per particle,
 * instead of a sphx_download and a host loop; and as a time series with nothing coming back to the host per step.  It also gives
 * sphx_render_fit its world rectangle and tells how full a box is before sphx_remove drains it.
 * Records: a call fills 1 + n_rects records.  Record 0 covers all N fluid particles (device order, the values sphx_download returns).
 *   Record 1 + k covers the particles whose position is in rects[k] by sphx_remove's predicate
 *     in(r, p) = p.x >= r.x0 && p.x < r.x1 && p.y >= r.y0 && p.y < r.y1
 *   (IEEE comparisons, half-open: a NaN coordinate is in no rectangle, infinite bounds are allowed, x0 > x1 is an empty rectangle).
 *   Rectangles may overlap; each record is independent of the others.  A particle with a non-finite x, y, vx or vy enters no sum and no
 *   extreme: it is counted in `nonfinite` (of a rectangle record when its position passes the predicate).  Of the `count` finite particles
 *   those with a finite density enter the density members and `density_count` — only while density[] belongs to the positions
 *   (density_valid == 1: the state in which sphx_sample_* succeeds); otherwise density[] is not read, density_count = 0, the density sums
 *   are 0 and the density extremes those of an empty record.
 * Arithmetic: every term is formed in float64 from the float32 values exactly as the member comments say; a product of two converted
 *   floats is exact in float64, so each term takes at most one rounding and fused and unfused evaluation give the same bits.  The ORDER
 *   of a summation is not part of the contract; each sum S of n terms t satisfies |S - exact| <= n * 2^-52 * sum|t| (any-order recursive
 *   summation errs by at most (n-1)u / (1 - (n-1)u) * sum|t|, u = 2^-53: less than half of that).  Counts, minima, maxima and max_speed_sq
 *   are exact; among zeros of either sign a minimum is -0 if one is present and a maximum +0 if one is present.
 * Determinism: two calls on the same state return identical bytes, on the host path and on the device-pointer path alike (no atomics:
 *   the grid and every order of addition are functions of N alone); a recorded frame equals the call made at that moment.
 * Physical quantities are the caller's: momentum = m * sum_vel, E_kin = m/2 * sum_speed_sq, E_pot = -m * (g . sum_pos), centre of mass
 *   = sum_pos / count, angular momentum about c = m * (sum_angular - (c.x * sum_vel[1] - c.y * sum_vel[0])), density variance =
 *   sum_density_sq / density_count - (sum_density / density_count)^2.
 * When allowed: sphx_fluid_stats wherever sphx_download is (a pending advection is applied first, as in sphx_render) and before any upload
 *   (N = 0: empty records); SPHX_ERR_NOT_READY between a step_begin and its step_finish (either solver).  Densities never make the call
 *   fail.  A tile context (sphx_tile_*, sphx_multi_tile_ctx) is refused with SPHX_ERR_INVALID_ARGUMENT: its arrays hold ghosts and miss
 *   the particles other tiles own.  A tiled run has sphx_multi_fluid_stats and sphx_multi_stats_* (below, with sphx_multi): the same
 *   records over the particles the tiles own, combined across the tiles.
 * Argument errors (SPHX_ERR_INVALID_ARGUMENT, the message names the argument): ctx, out or status NULL, rects NULL with n_rects > 0,
 *   n_rects > SPHX_STATS_MAX_RECTS, a NaN bound, unknown flag bits, a device `out` that is not 8-byte aligned.
 * SPHX_STATS_DEVICE_POINTERS: `out` is device memory on the context's device, 8-byte aligned; the call is enqueued on the context's
 *   stream and does not wait.  Without it: host memory; the call goes through a small device scratch (allocated on first use, freed in
 *   sphx_destroy) and returns when the records are written.  `rects` is host memory either way (copied).
 * Recording: after sphx_stats_record(rects, n_rects, max_frames, every) every every-th SUCCESSFULLY finished step (either solver, counted
 *   from the call; so also each step inside sphx_solver_simulation_steps) enqueues one frame of 1 + n_rects records behind its own
 *   kernels.  Nothing comes back to the host and nothing is synchronised.  The library keeps one sphx_stats_frame per frame on the host:
 *   step = finished steps since the call (1-based), dt = the dt given to that step_finish, n = the particle count at that moment.  A
 *   failed step takes no frame and does not count.  Once max_frames frames are stored, later frames are counted in `dropped`.
 *   max_frames == 0 stops and frees; every == 0 is SPHX_ERR_INVALID_ARGUMENT; a buffer (max_frames * (1 + n_rects) * 128 bytes) above
 *   64 MiB is SPHX_ERR_CAPACITY; a new sphx_stats_record discards the old recording.  sphx_stats_read copies the frames [first_frame,
 *   first_frame + n_frames) and waits for the stream; a range beyond `frames` is SPHX_ERR_INVALID_ARGUMENT.  Record, read: SPHX_ERR_NOT_READY
 *   inside an open step, a tile context is refused.
 * Lifetime: the recording belongs to the CONTEXT: sphx_upload, sphx_append, sphx_remove and sphx_state_load leave it alone (frames simply
 *   see the new particle set); sphx_state_save does not store it.
 * No side effects: all of this only reads the particle state.  A run with stats calls and a recording between its steps is bit-identical
 *   to the same run without them — every sphx_state_digest word, every sphx_step_stats field, sphx_last_flags — and a queued run-ahead
 *   pass stays valid.
 * Cost: two launches; pos, vel and (while valid) density are streamed once, rectangles are decided per wavefront (the particles are
 *   cell-sorted, so a wavefront that lies outside a rectangle skips it); DESIGN.md section 4i. */
#define SPHX_STATS_MAX_RECTS 8
enum { SPHX_STATS_DEVICE_POINTERS = 1u };
typedef struct sphx_stats_rec {      /* 128 bytes, every member naturally aligned */
    uint64_t count;                  /*   0: finite particles of this record */
    uint64_t nonfinite;              /*   8: particles with a non-finite x, y, vx or vy (in no sum, no extreme) */
    uint64_t density_count;          /*  16: of `count`, those whose density is finite (0 when !density_valid) */
    uint32_t density_valid;          /*  24: 1 iff density[] belonged to the positions (the state in which sphx_sample_* succeeds) */
    uint32_t reserved;               /*  28: 0 */
    double sum_pos[2];               /*  32: sum (double)x, sum (double)y */
    double sum_vel[2];               /*  48 */
    double sum_speed_sq;             /*  64: sum of t = (double)vx*(double)vx + (double)vy*(double)vy */
    double sum_angular;              /*  72: sum of (double)x*(double)vy - (double)y*(double)vx  (about the origin) */
    double sum_density;              /*  80 */
    double sum_density_sq;           /*  88: sum of (double)rho*(double)rho */
    double max_speed_sq;             /*  96: max of t; 0 for an empty record */
    float min_pos[2], max_pos[2];    /* 104, 112: +INFINITY / -INFINITY for an empty record */
    float min_density, max_density;  /* 120, 124: likewise */
} sphx_stats_rec;
typedef struct sphx_stats_frame { uint64_t step; float dt; uint32_t n; } sphx_stats_frame;   /* 16 bytes */
typedef struct sphx_stats_status { uint32_t n_rects, recording, max_frames, every, frames, dropped, reserved[2]; } sphx_stats_status;
int sphx_fluid_stats(sphx_ctx* ctx, const sphx_rect* rects /* host */, uint32_t n_rects, uint32_t flags, sphx_stats_rec* out /* [1 + n_rects] */);
int sphx_stats_record(sphx_ctx* ctx, const sphx_rect* rects /* host */, uint32_t n_rects, uint32_t max_frames, uint32_t every);
int sphx_stats_get_status(const sphx_ctx* ctx, sphx_stats_status* out);
int sphx_stats_read(sphx_ctx* ctx, uint32_t first_frame, uint32_t n_frames, sphx_stats_rec* out /* host, [n_frames][1 + n_rects] */,
                    sphx_stats_frame* info /* host, [n_frames], may be NULL */);

/* ---- gauges and probes: water levels along rays, and a per-step recorder of levels and point probes --------------------------------
 * What a dam-break study plots is a time series at fixed places: the water height at the gauges H1..H4, the position of the front along
 * the bed, the velocity at a few probe points.  sphx_gauge_levels samples rays on the device and reduces each ray to one record (the
 * highest sample inside the fluid and the crossing point behind it); sphx_probe_record stores such records, and sphx_sample_points'
 * outputs at fixed points, behind every every-th finished step without synchronising anything.
 * The gauge contract (all fp32, unfused, one rounding per operation):
 *   Samples: sample k of a gauge is the point (x0 + (float)k*dx, y0 + (float)k*dy), 0 <= k < n.  f_k is exactly what sphx_sample_points
 *     returns at that point for the chosen field (SPHX_GAUGE_FIELD_FRACTION: fraction, SPHX_GAUGE_FIELD_DENSITY: density), kernel_kind
 *     and state — the same device function, the same bits; for dx == 0 that is column 0 of sphx_sample_grid(x0, y0, any dx, dy, 1, n).
 *     `values`, when given, receives those bits, gauge after gauge.
 *   Inside test and counts: b_k = (f_k >= iso); a NaN value is outside.  first = the lowest k with b_k, last = the highest, inside = the
 *     number of k with b_k.  inside < last - first + 1 means a bubble or a detached splash on the ray.
 *   Crossing:
 *     0 <= last < n-1, with a = last and b = last+1:  t = (iso - f_a) / (f_b - f_a), (x, y) = (x_a + t*(x_b - x_a), y_a + t*(y_b - y_a)),
 *       f_last = f_a, f_next = f_b.  (f_b - f_a is never zero here: equal values compare alike with iso.)
 *     last == n-1 (the ray ends wet):  t = 0, (x, y) = sample n-1, f_last = f_(n-1), f_next = the word 0x7FC00000.
 *     nothing inside:  first = last = SPHX_GAUGE_NONE, inside = 0, and t, x, y, f_last, f_next are the word 0x7FC00000.
 *     The first row is sphx_surface_contour's crossing rule (a is the lower sample index): a vertical gauge at x0 returns, bit for bit,
 *     the point where the contour cuts the left edge of cell (0, last) of the lattice (x0, y0, any dx > 0, dy, 2, n).  A gauge with
 *     dy == 0 gives the position of the front along the bed.
 *   sphx_gauge_reduce is this rule over given values, as plain host code without a context (gauges[k].n values per gauge, gauge after
 *     gauge); the device agrees with it bit for bit.  It returns SPHX_ERR_INVALID_ARGUMENT for the argument errors below (and for
 *     values NULL with samples to read).
 *   Argument errors (SPHX_ERR_INVALID_ARGUMENT, the message names the argument): out NULL, gauges NULL with n_gauges > 0, n_gauges >
 *     SPHX_GAUGE_MAX, a gauge with n == 0 or n > 2^20, the sum of n above 2^24, a non-finite x0, y0, dx, dy or iso, an unknown
 *     kernel_kind, field or flag bit.  n_gauges == 0 succeeds.  Negative and zero steps are legal.  A ray that leaves the domain or the
 *     covered region never faults: its samples are sampling's zeros.
 *   When allowed, refusals, side effects: as sphx_sample_points (the same SPHX_ERR_NOT_READY rules and messages, a tile context is
 *     refused, the call only reads).  Two calls on one state return the same bytes: no atomic is used anywhere.
 *   SPHX_GAUGE_DEVICE_POINTERS: out and values are device pointers (out 4-byte aligned); the call is enqueued on the context's stream
 *     and does not wait.  Without it: host pointers, through a device scratch grown on demand and freed in sphx_destroy.  `gauges` is
 *     host memory either way (copied).
 * The recorder: after sphx_probe_record(points, m_points, gauges, n_gauges, ..., max_frames, every) every every-th SUCCESSFULLY finished
 *   step (either solver, counted from the call; so also each step inside sphx_solver_simulation_steps) enqueues one frame behind its own
 *   kernels: m_points sphx_probe_rec (sphx_sample_points' four outputs at the fixed points, reserved zero), then n_gauges
 *   sphx_gauge_rec.  Nothing comes back to the host and nothing is synchronised until the read.  The library keeps one
 *   sphx_stats_frame per frame on the host: step = finished steps since the call (1-based), dt = the dt given to that step_finish, n =
 *   the particle count at that moment.  A failed step takes no frame and does not count.  A finished step after which sampling is not
 *   allowed (a WCSPH step over zero fluid particles runs no build) takes no frame and is counted in `dropped`, as are the frames
 *   beyond max_frames.  max_frames == 0 stops and frees; every == 0, m_points + n_gauges == 0 with max_frames > 0, m_points >= 2^20 and
 *   the gauge errors above are SPHX_ERR_INVALID_ARGUMENT; a buffer (max_frames * (m_points + n_gauges) * 32 bytes) above 64 MiB is
 *   SPHX_ERR_CAPACITY; a new sphx_probe_record discards the old recording.  sphx_probe_read copies the frames [first_frame, first_frame +
 *   n_frames) and waits for the stream; a range beyond `frames` is SPHX_ERR_INVALID_ARGUMENT.  Record, read: SPHX_ERR_NOT_READY inside an
 *   open step, a tile context is refused.  Recording may be switched on before the first step: unlike the one-shot call it needs no
 *   sampleable state at the time of the call.
 *   Lifetime: points and gauges are copied at the call.  The recording belongs to the CONTEXT: sphx_upload, sphx_append, sphx_remove and
 *   sphx_state_load leave it alone; sphx_state_save does not store it.
 *   No side effects: a run with a recording (and gauge calls between its steps) is bit-identical to the same run without — every
 *   sphx_state_digest word, every sphx_step_stats field, sphx_last_flags — and a queued run-ahead pass stays valid.
 * Cost: a one-shot call is two launches behind ceil(n_gauges / 64) small ones that carry the gauges to the device; a recorded frame is
 *   three launches whatever the number of gauges; DESIGN.md section 4t. */
typedef struct sphx_gauge { float x0, y0, dx, dy; uint32_t n; uint32_t reserved[3]; } sphx_gauge;   /* 32 bytes: a ray of n samples */
typedef struct sphx_gauge_rec {       /* 32 bytes */
    uint32_t first, last, inside;     /* lowest / highest k with b_k, SPHX_GAUGE_NONE if none; number of k with b_k */
    float t;                          /* crossing parameter between last and last+1 */
    float x, y;                       /* crossing point */
    float f_last, f_next;             /* field at last and at last+1 */
} sphx_gauge_rec;
typedef struct sphx_probe_rec { float density, fraction, velocity[2]; uint32_t count; uint32_t reserved[3]; } sphx_probe_rec; /* 32 bytes */
typedef struct sphx_probe_status { uint32_t m_points, n_gauges, recording, max_frames, every, frames, dropped, reserved; } sphx_probe_status;
#define SPHX_GAUGE_NONE 0xFFFFFFFFu
#define SPHX_GAUGE_MAX 1024
enum { SPHX_GAUGE_FIELD_FRACTION = 0, SPHX_GAUGE_FIELD_DENSITY = 1 };
enum { SPHX_GAUGE_DEVICE_POINTERS = 1u };
int sphx_gauge_levels(sphx_ctx* ctx, const sphx_gauge* gauges /* host */, uint32_t n_gauges, int kernel_kind, int field, float iso,
                      uint32_t flags, sphx_gauge_rec* out /* [n_gauges] */, float* values /* [sum n], gauge after gauge, or NULL */);
int sphx_gauge_reduce(const float* values, const sphx_gauge* gauges, uint32_t n_gauges, float iso, sphx_gauge_rec* out);
int sphx_probe_record(sphx_ctx* ctx, const float* points_xy /* host */, uint32_t m_points, const sphx_gauge* gauges /* host */,
                      uint32_t n_gauges, int kernel_kind, int field, float iso, uint32_t max_frames, uint32_t every);
int sphx_probe_get_status(const sphx_ctx* ctx, sphx_probe_status* out);
int sphx_probe_read(sphx_ctx* ctx, uint32_t first_frame, uint32_t n_frames, sphx_probe_rec* points_out /* [n_frames][m_points] or NULL */,
                    sphx_gauge_rec* gauges_out /* [n_frames][n_gauges] or NULL */, sphx_stats_frame* info /* [n_frames] or NULL */);

/* Test aid for the zero-correction skip: cumulative numbers of correction workgroups that skipped their walk
 * (out[0]), that a flag inside their window stopped (out[1]) and that a flag behind an out-of-window table line stopped (out[2]; a workgroup
 * with a wavefront in the wide list format never looks further and is counted here too).
 * Collected only by a context created with SPHX_ZERO_SKIP_COUNT=1 in the environment (all zero otherwise); the skip itself is on by
 * default in a context of 4 M particles or more; SPHX_ZERO_SKIP=0 turns it off, =1 on at every size.  Waits for the stream. */
int sphx_debug_correction_counts(sphx_ctx* ctx, uint64_t out[3]);
/* Test aid for the quiet-scene exit of the same corrections, cumulative since sphx_create:
 * out[0] = workgroups that left through the quiet exit (each of them also counts in out[0] of sphx_debug_correction_counts),
 * out[1] = corrections the host queued in the decide-first form.  Collected only with SPHX_ZERO_SKIP_COUNT=1.  Waits for the stream. */
int sphx_debug_quiet_counts(sphx_ctx* ctx, uint64_t out[2]);
/* Test aid for the quiet take-over, cumulative since sphx_create:
 * out[0] = corrections queued in the thin form (counted by the host on every context);
 * out[1] = producers that took over — a neighbour build or compute_density_change that also stored the warm-start sums, a
 *          compute_density_error that also made the cell count.  Counted when the producer is queued: a build whose correction
 *          later runs the full form after all (its mark's number was taken by another iteration) is counted too;
 * out[2] = particles whose cell the recount of a marked thin density correction moved (collected only with SPHX_ZERO_SKIP_COUNT=1).
 * Waits for the stream.  Switches, read by sphx_create: SPHX_QUIET_TAKEOVER=0 (never) / 1 (default: under a loop's quiet hint,
 * wherever flags exist) / force (every first iteration with flags), SPHX_QUIET_TAKEOVER_DENSITY=0 (the divergence loop only),
 * SPHX_THIN_GRID=n (workgroups of a thin launch; default 2 048). */
int sphx_debug_takeover_counts(sphx_ctx* ctx, uint64_t out[3]);

/* Test aid for the rigid-motion form of the non-pressure pass: out[0] = passes queued in the rigid form,
 * out[1] = of those, the ones that found no mark and stored the uniform acceleration, out[2] = the ones that found a mark and ran
 * the full pass; cumulative since the context was created.  Waits for the stream.  Switch, read by sphx_create: SPHX_RIGID_SKIP=0
 * (never: the launches from before) / 1 (at every context size; default: from 4 M particles, where the flags exist) / force
 * (whatever the hint says). */
int sphx_debug_rigid_counts(sphx_ctx* ctx, uint64_t out[3]);
/* Test aid: the rigid form of the first density producer.  A rigid non-pressure pass that finds no mark leaves
 * the acceleration array unwritten, and the velocity prediction + compute_density_error behind it reads the uniform acceleration from
 * its arguments; a workgroup none of whose particles has a static neighbour leaves without a list word or a neighbour's record.
 * out[0] launches queued in that form (host count); with SPHX_ZERO_SKIP_COUNT=1 also out[1] workgroups that took the fluid-only exit,
 * out[2] workgroups that walked with the uniform acceleration, out[3] launches that found no verdict (the pass had found a mark and
 * filled the array: today's loads).  Cumulative; waits for the stream.  Switch, read by sphx_create: SPHX_RIGID_PREDICT=0 (the rigid
 * pass fills the array: the launches from before) / accel (no exit: every workgroup walks) / default: both, wherever the rigid pass
 * is queued. */
int sphx_debug_rigid_predict_counts(sphx_ctx* ctx, uint64_t out[4]);
/* Test aid: the acceleration array as the latest non-pressure pass left it, in sorted order — between two DFSPH steps the pass that
 * ran ahead for the next one (where a rigid pass left the array to its reader, the fill it left out is queued first; the course of
 * the run does not change).  out_xy holds 2 * N floats.  Waits for the stream. */
int sphx_debug_download_accel(sphx_ctx* ctx, float* out_xy);
/* Test aid: sphx_download's arrays between sphx_wcsph_step_begin and sphx_wcsph_step_finish, where sphx_download is refused like in
 * every open step: the re-sorted, leap-frogged positions, the velocities at the half step (wscsph.rs:148), the Poly6 densities and
 * the ids.  Any pointer may be NULL.  Outside a WCSPH step: SPHX_ERR_NOT_READY.  Waits for the stream; the course of the run does not
 * change. */
int sphx_debug_download_wcsph_half_step(sphx_ctx* ctx, float* pos_xy, float* vel_xy, float* density, uint32_t* particle_id);

/* ---- Solver trait (solver/mod.rs:12-18) ---------------------------------------------------------------------- */
/* Solver::clear_cached_data (dfsph.rs:406-412) */
int sphx_clear_cached(sphx_ctx* ctx);
/* Solver::simulation_step is two-phase because the reference calls back into the caller-owned TimeManager mid-step:
 *   phase A = dfsph.rs:419-477 (warm-up if needed, non-pressure accelerations + XSPH with dt_prev =
 *             time_manager.simulation_step().as_secs_f32(), max |v + a*dt_prev|) -> *out_vmax = sqrt(max)
 *   host    = dt = time_manager.update_simulation_step(2*radius, vmax).as_secs_f32()   (dfsph.rs:478-480)
 *   phase B = dfsph.rs:484-524 (predict, constant-density loop, advect, re-grid, density+alpha, divergence loop, swap) */
int sphx_step_begin(sphx_ctx* ctx, float dt_prev, float* out_vmax);
int sphx_step_finish(sphx_ctx* ctx, float dt, sphx_step_stats* out_stats);

/* The law the caller's TimeManager is about to apply to vmax (TimeManager::update_simulation_step, timemanager.rs:252-279,
 * with the public TimerConfig of timemanager.rs:10-60 and the current TimeManager::simulation_step()).  Handing it to phase A
 * lets the device derive the same dt right behind its vmax reduction and put the start of phase B (velocity prediction, first
 * constant-density iteration) on the stream before the host has even read vmax: the GPU no longer idles for the host round trip.
 * The host side is unchanged — it still calls update_simulation_step with *out_vmax and passes the result to
 * sphx_step_finish, which verifies bit for bit that both arrived at the same dt (SPHX_ERR_INVALID_ARGUMENT otherwise; the
 * device state is then stale and must be uploaded again). */
typedef struct sphx_timer_law {
    uint32_t adaptive;            /* SimulationStepConfig::Adaptive (1) or ::Fixed (0: dt stays simulation_step_ns) */
    float cfl_factor;             /* AdaptiveTimeStep cfl factor (main.rs:126) */
    float particle_diameter;      /* 2 * particle_radius (dfsph.rs:479) */
    uint32_t reserved;
    uint64_t timestep_min_ns;     /* main.rs:124 */
    uint64_t timestep_max_ns;     /* main.rs:123 */
    uint64_t simulation_step_ns;  /* TimeManager::simulation_step() before the update, in nanoseconds */
} sphx_timer_law;
int sphx_step_begin_law(sphx_ctx* ctx, float dt_prev, const sphx_timer_law* law, float* out_vmax); /* law == NULL: sphx_step_begin */

/* WCSPHSolver::simulation_step (solver/wscsph.rs:126-179), the second Solver behind the same boundary,
 * two-phase for the same reason:
 *   phase A = leap frog 1 with dt = time_manager.simulation_step() (:138-149), update_neighborhood_datastructure (:152),
 *             update_densities(Poly6) (:153), update_accellerations (:59-118, :154), max |v + a*dt| (:158-161) -> *out_vmax
 *   host    = dt = time_manager.update_simulation_step(2*radius, vmax).as_secs_f32()   (:162-164)
 *   phase B = leap frog 2 (:168-177)
 * Constants as WCSPHSolver::new (:31-49): Poly6 density kernel, Spiky pressure kernel, XSPH viscosity (or the physical model: sphx_params.viscosity_model), Tait gamma 7,
 * set_compressibility(0.01, 1.0), boundary_force_factor 1.  sphx_clear_cached also drops the accelerations (:122-124).
 * One context runs one solver: the DFSPH and the WCSPH step share the acceleration array. */
int sphx_wcsph_step_begin(sphx_ctx* ctx, float dt, float* out_vmax);
int sphx_wcsph_step_finish(sphx_ctx* ctx, float dt, sphx_step_stats* out_stats);

/* ---- pieces of the path the reference exposes on FluidParticleWorld (driven by benches/) --------------------- */
/* FluidParticleWorld::update_neighborhood_datastructure(vec![], vec![]) (fluidparticleworld.rs:235-261) */
int sphx_update_neighborhood(sphx_ctx* ctx);
/* FluidParticleWorld::update_densities(kernel) (fluidparticleworld.rs:197-231) */
int sphx_update_densities(sphx_ctx* ctx, int kernel_kind);
/* DFSPHSolver::compute_alpha_factors (dfsph.rs:68-97) on the current lists */
int sphx_compute_alpha(sphx_ctx* ctx);

/* ---- parity/inspection (not on the hot path) ------------------------------------------------------------------ */
/* DFSPHSolver::{alpha_values, warmstart_kappa, warmstart_stiffness} (dfsph.rs:36-40); any pointer may be NULL */
int sphx_download_solver_state(sphx_ctx* ctx, float* alpha, float* kappa, float* stiffness);
/* NeighborLists (neighborhood_search.rs:262-300, 433-449) in canonical form: counts[2*i] = count_dynamic,
 * counts[2*i+1] = count_total; lists = all particles' lists concatenated in particle order (the reference's
 * start_index is thread-schedule dependent and is not part of the contract).  Either pointer may be NULL. */
int sphx_download_neighbors(sphx_ctx* ctx, uint16_t* counts, uint32_t* lists, uint64_t* out_total_entries);
/* CompactMortonCellGrid::cells (neighborhood_search.rs:34-37,142-165) incl. the sentinel; which: 0 dynamic, 1 static.
 * Pass NULL arrays to query the count. */
int sphx_download_cells(sphx_ctx* ctx, int which, uint32_t* first_particle, uint32_t* cidx, uint32_t* out_count);
/* SPHX_FLAG_* bits raised since the latest sphx_step_begin (also by the stand-alone sphx_update_neighborhood) */
uint32_t sphx_last_flags(const sphx_ctx* ctx);
/* the cell table behind the grid (which: 0 dynamic, 1 static): out[0] = covered 64x64-cell blocks, out[1] = table
 * entries (= 4096 x blocks: what every build's histogram scan runs over), out[2], out[3] = extent of the block directory */
int sphx_grid_info(const sphx_ctx* ctx, int which, uint32_t* out4);
/* derived kernel constants: out[0..2] = Wendland {h_inv, normalizer, normalizer_grad} (wendland_quintic_c2.rs:24-30),
 * out[3..5] = Poly6 {hsq, normalizer, normalizer_grad} (poly6.rs:16-23) */
int sphx_get_constants(const sphx_ctx* ctx, float* out6);
/* the viscosity model the context runs (any pointer may be NULL): the model, fluid_viscosity and the Viscosity kernel's
 * normalizer_laplacian = 360 / (29 pi h^5) (viscosity.rs:24).  A shim calls it once after sphx_create: a library older than
 * these fields does not export it (and would ignore the reserved words the fields occupy). */
int sphx_get_viscosity(const sphx_ctx* ctx, uint32_t* model, float* fluid_viscosity, float* normalizer_laplacian);


/* ---- spatial tiles (multi-GPU) ------------------------------------------------------------------------------
 * The reference has no distributed path; these entry points are the device half of the build's own domain decomposition.
 * One context = one tile: the cells with cell_lo <= c < cell_hi along `axis` (0 = x, 1 = y) are OWNED, a halo of `halo_cells`
 * cells on each side holds copies (ghosts) of the neighbours' particles.  The host driver (sphx_multi_* below — csrc/sphx_tiles.cpp; tests/tiles_reference.py is its Python
 * reference implementation) runs the sub-steps below in the order of dfsph.rs:414-525, all-reduces the three
 * per-step scalars, and once per step — between advect and re-grid — exchanges 32-byte halo records with the two spatial
 * neighbours (RCCL send/recv on the device buffers).  With a halo wider than the number of neighbour traversals between two
 * exchanges, ghost values are recomputed locally instead of being exchanged per sub-step.
 * In tile mode the warm-start arrays travel with their particle (a slot-bound array has no meaning across tiles). */
int sphx_reserve(sphx_ctx* ctx, uint32_t capacity); /* device capacity in particles (owned + ghosts + 2 halo buffers); before upload */
int sphx_tile_configure(sphx_ctx* ctx, int axis, uint32_t cell_lo, uint32_t cell_hi, uint32_t halo_cells, int has_left, int has_right);
/* General form ("4 GPUs: 2x2 tiles"): the context owns the cell rectangle *own; peers[] are the rectangles of the
 * tiles that touch it by an edge or a corner (<= SPHX_MAX_TILE_PEERS), in the order of the buffers given to sphx_tile_pack_n /
 * sphx_tile_apply_n.  A strip is a rectangle spanning the whole other axis; sphx_tile_configure/pack/apply are that special case. */
#define SPHX_MAX_TILE_PEERS 8
typedef struct sphx_tile_rect { uint32_t x0, x1, y0, y1; } sphx_tile_rect; /* cells, half-open */
int sphx_tile_configure_rect(sphx_ctx* ctx, const sphx_tile_rect* own, uint32_t halo_cells, const sphx_tile_rect* peers, uint32_t n_peers);
int sphx_tile_pack_n(sphx_ctx* ctx, void* const* d_send, uint32_t n_send, uint32_t cap_records);         /* n_send == n_peers */
int sphx_tile_apply_n(sphx_ctx* ctx, const void* const* d_recv, uint32_t n_recv, uint32_t cap_records);  /* entries may be NULL */
int sphx_tile_advect_pack_n(sphx_ctx* ctx, float dt, void* const* d_send, uint32_t n_send, uint32_t cap_records); /* sphx_sub_advect + sphx_tile_pack_n in one pass */
int sphx_tile_upload(sphx_ctx* ctx, const float* pos_xy, const float* vel_xy, const uint32_t* ids, uint32_t n); /* owned particles, global ids < 2^31 */
#define SPHX_HALO_RECORD_BYTES 32 /* {float4 pos+vel, u32 id, f32 kappa, f32 stiffness, u32 pad}; record 0 = header (count in .id) */
int sphx_tile_pack(sphx_ctx* ctx, void* d_send_left, void* d_send_right, uint32_t cap_records);              /* DEVICE buffers, (1+cap)*32 B */
int sphx_tile_apply(sphx_ctx* ctx, const void* d_from_left, const void* d_from_right, uint32_t cap_records); /* DEVICE buffers or NULL */
int sphx_tile_count_kept(sphx_ctx* ctx); /* between pack and apply: cell count of the kept particles, overlapping the exchange */
int sphx_sub_regrid(sphx_ctx* ctx, uint32_t* out_n_local);                 /* dfsph.rs:512-518 on owned + ghosts */
/* The same, and the neighbour build also does the first compute_density_change (dfsph.rs:249-280) of the divergence loop that
 * follows: the next sphx_sub_iteration(divergence = 1, first = 1) then skips that pass.  Only for a loop that starts WITHOUT a
 * warm start (sphx_sub_warmstart after this call is refused: the pass has already zeroed the warm-start values). */
int sphx_sub_regrid_div(sphx_ctx* ctx, uint32_t* out_n_local);
/* The other case: the divergence loop that follows starts WITH a warm start (dfsph.rs:354-360); the neighbour build applies it, and
 * the sphx_sub_warmstart(divergence = 1) call that follows returns without launching anything. */
int sphx_sub_regrid_warm(sphx_ctx* ctx, uint32_t* out_n_local);
/* The tile loop's run-ahead over the step boundary: arms the NEXT sphx_sub_iteration to queue the next step's non-pressure pass (with
 * dt_prev = dt_prev_of_next_step) and the publish of its maximum behind its own kernels; the next sphx_sub_nonpressure with the same
 * dt_prev adopts the result if nothing has touched the context in between, and simply runs again otherwise. */
int sphx_sub_run_ahead(sphx_ctx* ctx, float dt_prev_of_next_step);
/* Tile mode: which warm-start arrays (warmstart_kappa, warmstart_stiffness) the re-grids move with their particles (default: both).
 * An array the next solver loop zeroes before it reads it (no warm start: dfsph.rs:199 / :354) need not travel. */
int sphx_tile_carry_warmstart(sphx_ctx* ctx, int kappa, int stiffness);
/* Tile mode, for callers that run sphx_tile_advect_pack_n -> exchange -> sphx_tile_apply_n -> sphx_sub_regrid* back to back: the packing
 * pass classifies, counts and sends the advected particles but leaves the records of the particles the tile keeps to the re-grid's
 * gather, which applies the same x += v* dt while it moves them (24 bytes per particle less in the packing pass).  Any other entry
 * point that looks at the records in between applies the pending advection first. */
int sphx_tile_defer_advect(sphx_ctx* ctx, int on);
/* Tile mode statistics: halo packs (sphx_tile_advect_pack_n) that found their particles classified by the density loop's last
 * correction — send counts per workgroup, kept / retired, cell count (SPHX_TILE_FUSE_CLASS=0 turns that off) — and only visited
 * the workgroups that send something. */
int sphx_tile_band_packs(const sphx_ctx* ctx, uint32_t* out);
/* The record counts in the headers of the send buffers the last sphx_tile_pack_n / sphx_tile_advect_pack_n filled (clamped to
 * cap_records), on the host: waits for the packing kernels (one small device-to-host copy per peer).  The caller may then move
 * (1 + out_counts[k]) * 32 bytes per peer instead of the buffers' capacity. */
int sphx_tile_send_counts(sphx_ctx* ctx, void* const* d_send, uint32_t n_send, uint32_t cap_records, uint32_t* out_counts);
int sphx_sub_nonpressure(sphx_ctx* ctx, float dt_prev, float* out_vmax_sq); /* dfsph.rs:436-477; max over OWNED particles */
int sphx_sub_predict(sphx_ctx* ctx, float dt);                             /* dfsph.rs:484-492 */
int sphx_sub_warmstart(sphx_ctx* ctx, int divergence, float dt);           /* dfsph.rs:199-205 / :354-360 */
int sphx_sub_iteration(sphx_ctx* ctx, int divergence, float dt, int first, double* out_err_sum, uint64_t* out_n_owned); /* :217-221 / :372-377 */
int sphx_sub_advect(sphx_ctx* ctx, float dt);                              /* dfsph.rs:499-510 */
/* sphx_sub_predict followed by sphx_sub_iteration(divergence = 0, first = 1) in one call, for a density loop that starts without a
 * warm start (dfsph.rs:199): one list walk does both (the prediction costs no pass of its own).  Same results as the two calls. */
int sphx_sub_predict_iteration(sphx_ctx* ctx, float dt, double* out_err_sum, uint64_t* out_n_owned);


/* ---- multi-GPU solver behind the Solver boundary ("device list ... internally may drive 1-8 GPUs") ----------------
 * The reference's caller holds ONE Box<dyn Solver> (main.rs:50) and calls simulation_step(&mut world, &mut time_manager)
 * (solver/mod.rs:12-18, main.rs:279).  sphx_multi is that one object over several GPUs: it cuts the domain into tiles (strips along
 * the longer side; 2 x N/2 rectangles on 4 tiles), owns one context per tile and runs the whole tile step loop — ring-budget halo,
 * one exchange per step, adaptive band, re-partitioning — inside the library.  Same two-phase step as sphx_step_begin/finish. */
typedef struct sphx_multi sphx_multi;
enum { SPHX_LAYOUT_AUTO = 0, SPHX_LAYOUT_STRIPS = 1, SPHX_LAYOUT_GRID = 2 };
typedef struct sphx_multi_options {
    uint32_t halo_cells;       /* widest ghost band in cells (16); the band in use follows the ring budget unless fixed_halo */
    uint32_t fixed_halo;       /* 1: always exchange the full band */
    uint32_t rebalance_every;  /* steps between re-partitions of the cuts (16; 0 = never) */
    uint32_t layout;           /* SPHX_LAYOUT_* (auto: 2x2 on 4 tiles, strips otherwise) */
    uint32_t cap_records;      /* records per halo buffer (0 = estimated from the uploaded scene) */
    uint32_t overlap_exchange; /* 1: halo records on a second stream, the re-grid's cell count of the kept particles meanwhile */
    uint32_t reserved[2];
} sphx_multi_options;
/* Communicator supplied by the caller for one tile of a multi-process run (NULL: the built-in one — grouped ncclSend/ncclRecv over
 * RCCL for the halo records, the shared-memory all-reduce below for the scalars).  exchange: send d_send[k] to rank peers[k] and
 * receive d_recv[k] from it, `bytes` each, DEVICE buffers, ordered on hip_stream (no host synchronisation required of the caller's
 * caller).  allreduce: op 0 = sum, 1 = max over n <= 8 doubles; every rank must receive the same bits. */
typedef struct sphx_comm_ops {
    void* user;
    int rank, world;
    int (*exchange)(void* user, const int* peers, int n_peers, void* const* d_send, void* const* d_recv, size_t bytes, void* hip_stream);
    int (*allreduce)(void* user, const double* in, int n, int op, double* out);
    /* optional (may be NULL): this rank has failed and will not take part in further calls — release the ranks waiting for it */
    void (*abort)(void* user);
} sphx_comm_ops;
typedef struct sphx_multi_info_t {
    uint32_t world, local_tiles, halo_now, halo_max, peers, n_local, cap_records, grid_layout;
    int32_t axis;
    uint32_t band_packs; /* of tile 0's halo exchanges: how many packed from the classification its last density correction had made
                            (only the workgroups inside a send band were visited again) */
    uint64_t exchanges, rebalances;
    /* the local tiles' latest neighbour build (measured, not assumed): particles it ran over (owned + ghosts), list entries, and
     * entries outside the workgroup windows — mean list length = neighbor_entries / build_particles */
    uint64_t build_particles, neighbor_entries, remote_entries;
    uint64_t owned_local; /* particles the local tiles own */
    char transport[96];
    /* tile 0's halo exchanges so far, bytes it sent to all its peers together: what its packing pass filled ((1 + records) * 32 per
     * peer) and what travelled (the same rounded up to 64 KiB when the record counts were exchanged first, else the buffers' capacity) */
    uint64_t halo_bytes_packed, halo_bytes_sent;
    double ownership_seconds; /* set-up, tile 0: cell, owner and send-band count of every particle of the global scene (host threads) */
} sphx_multi_info_t;
int sphx_multi_default_options(sphx_multi_options* out);
/* all tiles in this process: tile r runs on HIP device devices[r] (a device may appear more than once); one host thread per tile */
int sphx_multi_create(const sphx_params* params, const int* devices, int n_devices, const sphx_multi_options* opt, sphx_multi** out);
/* ONE tile (rank of world) of a one-process-per-GPU run; comm == NULL: built-in RCCL + shared memory, `job` names the shared segment
 * (unique per run, e.g. the rendezvous port) */
int sphx_multi_create_rank(const sphx_params* params, int device, const sphx_comm_ops* comm, const char* job, int rank, int world,
                           const sphx_multi_options* opt, sphx_multi** out);
void sphx_multi_destroy(sphx_multi* m);
const char* sphx_multi_last_error(const sphx_multi* m); /* m may be NULL: the last creation error */
/* optional explicit cuts (cells) instead of the particle-count quantiles of the uploaded scene: strips along axis, or nx columns
 * (xcuts[nx+1]) each cut again at its own ycuts[ix*(ny+1) ..] */
int sphx_multi_set_layout(sphx_multi* m, int axis, const uint32_t* cuts, uint32_t n_cuts);
int sphx_multi_set_grid_layout(sphx_multi* m, uint32_t nx, uint32_t ny, const uint32_t* xcuts, const uint32_t* ycuts);
int sphx_multi_set_boundary(sphx_multi* m, const float* xy, uint32_t n);  /* the GLOBAL boundary; every tile clips its part */
/* the GLOBAL particle arrays (every rank of a multi-process run passes the same ones; ids == NULL: 0..n-1); includes the warm-up
 * block of dfsph.rs:419-428 */
int sphx_multi_upload(sphx_multi* m, const float* pos_xy, const float* vel_xy, const uint32_t* ids, uint32_t n);
int sphx_multi_clear_cached(sphx_multi* m);                                           /* Solver::clear_cached_data */
int sphx_multi_step_begin(sphx_multi* m, float dt_prev, float* out_vmax);             /* dfsph.rs:419-477, vmax over ALL tiles */
int sphx_multi_step_finish(sphx_multi* m, float dt, sphx_step_stats* out_stats);      /* dfsph.rs:484-524 */
int sphx_multi_synchronize(sphx_multi* m);
uint64_t sphx_multi_num_owned(const sphx_multi* m);
/* owned particles of the local tiles (in-process: all particles), tile after tile; *inout_n: capacity in, count out */
int sphx_multi_download(sphx_multi* m, float* pos_xy, float* vel_xy, float* density, uint32_t* ids, uint64_t* inout_n);
int sphx_multi_info(const sphx_multi* m, sphx_multi_info_t* out);
sphx_ctx* sphx_multi_tile_ctx(sphx_multi* m, uint32_t local_tile); /* inspection (neighbours, cells, profiling) */

/* ---- fluid statistics of a tiled run (csrc/sphx_stats.inc, csrc/sphx_tiles.cpp, csrc/sphx_stats_merge.hpp) ---------------------------------
 * The records of sphx_fluid_stats (above: members, terms, rectangle predicate, arithmetic) for a run that is cut into tiles, without a
 * sphx_multi_download: every tile streams its local arrays once — pos, vel, density and particle_id, 24 bytes per particle — and keeps
 * the particles it OWNS (bit 31 of the id in the tile's arrays); a ghost enters no count, no sum, no extreme and no rectangle.  Every
 * particle of the run is owned by exactly one tile.
 * Combination: record r of the whole fluid is the fold of the tiles' records r in ASCENDING TILE RANK, ((t0 (+) t1) (+) t2) ..., with the
 *   a (+) b of the device's own reduction: each sum a + b in this order, integer addition for the counts, minimum / maximum for the
 *   extremes (among zeros of either sign a minimum is -0 if one is present, a maximum +0), fmax for max_speed_sq; density_valid is the AND
 *   over the tiles.  A tile that owns nothing contributes the empty record (zero sums and counts, +INFINITY / -INFINITY extremes).
 * Contract: counts, minima, maxima and max_speed_sq are exact.  Each sum is within n * 2^-52 * sum|t| of the exact one, n the number of
 *   terms of the WHOLE fluid's sum — the bound of sphx_fluid_stats is stated for any order of summation and so covers the fold.  Two calls
 *   on one state return identical bytes.  For every tiling of the same particle set (and the single context holding it) the counts, extremes
 *   and max_speed_sq are the same and the sums agree within that bound of the exact value; bitwise equality of the sums ACROSS tilings is not
 *   promised.
 * sphx_multi_fluid_stats(m, rects, n_rects, flags = 0, out, out_tiles): out (host, [1 + n_rects]) receives the whole fluid; out_tiles
 *   (host, [world][1 + n_rects], may be NULL) every tile's own records in ascending tile rank.  In-process (sphx_multi_create): every tile
 *   enqueues on its own stream and device, then the records are copied back and folded on the host.  Rank mode (sphx_multi_create_rank):
 *   the call is COLLECTIVE — every rank calls it with the same arguments — and every rank receives the same bytes, out_tiles included; the
 *   records cross the ranks bit for bit (as integers below 2^32, never as doubles a transport might renormalise).
 * When allowed: after sphx_multi_upload and after every finished step; SPHX_ERR_NOT_READY between sphx_multi_step_begin and _finish and
 *   before the first sphx_multi_upload (record and read too; behind a solver object the first simulation step uploads).
 *   density_valid is 1 in both states (the warm-up block of the upload and every step recompute the densities after the re-grid).
 *   SPHX_ERR_INVALID_ARGUMENT: m or out NULL, the rectangle errors of sphx_fluid_stats, any flags bit, more than 64 tiles.
 * Recording: after sphx_multi_stats_record(rects, n_rects, max_frames, every) every every-th SUCCESSFULLY finished multi step (from
 *   sphx_multi_step_finish or inside sphx_multi_simulation_step(s), counted from the call) makes every tile enqueue one frame of its own
 *   records into its own device buffer, behind that step's kernels.  Nothing comes back to the host and nothing is synchronised.
 *   sphx_stats_frame: step = finished steps since the call (1-based), dt = that step's dt, n = the owned count of the whole run as the
 *   step's last all-reduce left it.  Limits and semantics are those of sphx_stats_record, per tile: 64 MiB (SPHX_ERR_CAPACITY),
 *   max_frames == 0 stops and frees, every == 0 is SPHX_ERR_INVALID_ARGUMENT, a new call discards the old recording, frames beyond
 *   max_frames are counted in `dropped`.  The recording survives sphx_multi_upload and re-partitioning.  sphx_multi_stats_read copies the
 *   tiles' frames [first_frame, first_frame + n_frames), folds each frame as above and waits for the tiles' streams; it is collective in
 *   rank mode (four meetings of the ranks per record: meant for the end of a run, not for every step); a range beyond `frames` is
 *   SPHX_ERR_INVALID_ARGUMENT.  A recorded frame equals the sphx_multi_fluid_stats call made at that moment.
 * No side effects: all of this only reads the tiles' state (a queued run-ahead pass stays valid, the sweep direction is put back).  A run
 *   with stats calls and a recording between its steps is bit-identical to the same run without: everything sphx_multi_download returns,
 *   every sphx_step_stats field, sphx_multi_info().exchanges.
 * One tile: sphx_tile_fluid_stats has the arguments, flags, errors and device-pointer rule of sphx_fluid_stats, is accepted ONLY on a tile
 *   context (a plain one: SPHX_ERR_INVALID_ARGUMENT) and covers the particles that tile owns; SPHX_ERR_NOT_READY between a halo exchange
 *   and the tile's re-grid.  sphx_tile_stats_record / _frame / _read are the seam the multi recorder is built on (INTERNAL, like the other
 *   sphx_tile_* calls); sphx_stats_get_status reads a tile's recording too.
 * Cost: per tile the two launches of sphx_fluid_stats, 24 instead of 20 bytes per local particle; DESIGN.md section 4i. */
int sphx_tile_fluid_stats(sphx_ctx* tile_ctx, const sphx_rect* rects /* host */, uint32_t n_rects, uint32_t flags, sphx_stats_rec* out /* [1 + n_rects] */);
int sphx_tile_stats_record(sphx_ctx* tile_ctx, const sphx_rect* rects /* host */, uint32_t n_rects, uint32_t max_frames, uint32_t every);
int sphx_tile_stats_frame(sphx_ctx* tile_ctx, float dt, uint32_t n_global); /* one finished step: a frame if the recording is due */
int sphx_tile_stats_read(sphx_ctx* tile_ctx, uint32_t first_frame, uint32_t n_frames, sphx_stats_rec* out /* host */, sphx_stats_frame* info /* may be NULL */);
int sphx_multi_fluid_stats(sphx_multi* m, const sphx_rect* rects /* host */, uint32_t n_rects, uint32_t flags /* 0 */,
                           sphx_stats_rec* out /* host, [1 + n_rects]: the whole fluid */,
                           sphx_stats_rec* out_tiles /* host, [world][1 + n_rects], may be NULL: per tile, ascending tile rank */);
int sphx_multi_stats_record(sphx_multi* m, const sphx_rect* rects /* host */, uint32_t n_rects, uint32_t max_frames, uint32_t every);
int sphx_multi_stats_get_status(const sphx_multi* m, sphx_stats_status* out);
int sphx_multi_stats_read(sphx_multi* m, uint32_t first_frame, uint32_t n_frames, sphx_stats_rec* out /* host, [n_frames][1 + n_rects] */,
                          sphx_stats_frame* info /* host, [n_frames], may be NULL */);
/* ---- following particles by id in a tiled run (csrc/sphx_tiles.cpp; device pass csrc/sphx_track.inc, host merge csrc/sphx_track_merge.hpp) ----
 * sphx_track_* / sphx_download_by_id for a sphx_multi, without sphx_multi_download: every tile streams its particle_id[] once on its own
 * device and answers for the particles it OWNS; the host folds the tiles' parts.
 * Rule for one tile: a particle answers for id i iff bit 31 of its particle_id word is set (the tile owns it) and the other 31 bits are i.
 *   A ghost never answers; an id >= 2^31 is always absent.  Within a tile the HIGHEST slot answers (sphx_track_*'s rule); if several tiles
 *   hold an id — only a state loaded with repeated ids has that — the greatest (tile rank, slot) wins.
 * Values: sphx_multi_track_set hands over m ids (host memory, copied; any order; duplicates allowed and answered alike; m == 0 clears the
 *   set).  sphx_multi_track_fetch gives for the k-th id in the caller's order: tile[k] = the global rank of the tile that owns it, slot[k] =
 *   its index in that tile's sphx_download order, pos / vel / density = the exact bits that tile's arrays hold — the bits
 *   sphx_multi_download returns for that id.  An absent id has tile = slot = SPHX_TRACK_ABSENT and the word 0x7FC00000 in every float.  Any
 *   subset of the outputs gives the same bits.  An empty set is a successful no-op.
 * sphx_multi_download_by_id: the same for the ids first_id + k, k < count; *out_present = the ids found.  first_id + count may reach 2^32
 *   and no more; count == 0 is a successful no-op (*out_present = 0).  After an unedited sphx_multi_upload with ids == NULL, first_id = 0
 *   and count = n give the particles in upload order.  A tile appends one packed 32-byte record per owned particle of the window to a
 *   buffer sized from its owned count (the order in the buffer is undefined, the scattered result is not): about 32 bytes per particle of
 *   the window cross the bus in all, not world * count * 28.
 * In-process (sphx_multi_create): the answer is complete.  Rank mode (sphx_multi_create_rank): every call is LOCAL and communicates
 *   nothing; it returns this rank's part — an id another rank owns is absent, tile[] says which are present — and every rank must make
 *   the same set and record calls.  The caller moves the parts with its own transport and folds them with sphx_track_merge /
 *   sphx_track_merge_frames (the pattern of sphx_multi_render_layer / sphx_render_merge).
 * sphx_track_merge(m, parts, n_parts, out, out_present): pure host code, no GPU.  Every part is a sphx_multi_track_out of m entries with
 *   tile and slot present (SPHX_ERR_INVALID_ARGUMENT otherwise, or if out asks for an array a part lacks); entry k of out is taken from
 *   the part with the greatest (tile[k], slot[k]) among those whose tile[k] is not SPHX_TRACK_ABSENT (equal pairs: the earlier part), or
 *   is absent.  n_parts == 0 gives an all-absent answer.  sphx_track_merge_frames(n, parts, parts_tile, n_parts, out, out_tile): the same
 *   for n = n_frames * m frame entries {x, y, vx, vy} and their tile words (the greatest tile wins; out_tile may be NULL).
 * Recording: after sphx_multi_track_record(max_frames, every) every every-th SUCCESSFULLY finished multi step (sphx_multi_step_finish, and
 *   each step inside sphx_multi_simulation_step(s); counted from the call) makes every tile enqueue one frame behind that step's kernels:
 *   per distinct tracked id {x, y, vx, vy} and a presence word (the slot, or SPHX_TRACK_ABSENT — never inferred from the floats: a
 *   particle may carry 0x7FC00000), 20 bytes.  Nothing comes back to the host and nothing is synchronised; a failed step takes no frame
 *   and does not count.  max_frames * (distinct ids) * 20 bytes per tile may not exceed 1 GiB (SPHX_ERR_CAPACITY); frames beyond
 *   max_frames are counted in `dropped`; max_frames == 0 stops and frees; every == 0 is SPHX_ERR_INVALID_ARGUMENT; recording with an
 *   empty set is SPHX_ERR_NOT_READY.  sphx_multi_track_set and _record discard an earlier recording on every tile or on none.
 *   sphx_multi_track_read folds the frames [first_frame, first_frame + n_frames) into out[n_frames][m][4] (caller's order, absent = four
 *   0x7FC00000 words) and out_tile[n_frames][m] (owning tile or SPHX_TRACK_ABSENT; may be NULL); a range beyond `frames` is
 *   SPHX_ERR_INVALID_ARGUMENT.  A frame equals the sphx_multi_track_fetch made at that moment.
 * Lifetime: the set and the recording belong to the MULTI.  They survive migration, re-partitioning, sphx_multi_append / _remove (a removed
 *   id becomes absent, an appended id that is in the set is found), sphx_multi_state_load and sphx_multi_upload (the set keeps its numbers).
 * When allowed: after the first sphx_multi_upload or sphx_multi_state_load; SPHX_ERR_NOT_READY before it, between sphx_multi_step_begin
 *   and _finish and on a multi whose collective step has failed.  SPHX_ERR_INVALID_ARGUMENT (sphx_multi_last_error names the argument):
 *   m > SPHX_TRACK_MAX_IDS, ids NULL with m > 0, out NULL or every pointer in it NULL, any flags bit, first_id + count > 2^32, out of
 *   sphx_multi_track_read NULL with n_frames > 0.  A refused call touches no tile.
 * No side effects: only reads.  Every sphx_multi_state_digest word, every sphx_step_stats field and the timer are the same with and without
 *   a set, fetches, by-id downloads and a recording; a queued run-ahead pass stays valid, the sweep direction is put back.
 * One tile (INTERNAL, like the other sphx_tile_* calls; a plain context is refused with SPHX_ERR_INVALID_ARGUMENT): sphx_tile_track_install
 *   takes the tables of ONE track_build (csrc/sphx_track_set.hpp) — the same for every tile; unique == 0 clears — and drops the tile's
 *   recording.  _fetch_enqueue queues look-up and gather on the tile's stream, _fetch copies back per distinct id the slot word, {x, y, vx,
 *   vy} and the density.  _window_enqueue(first_id, count <= 2^22, cap_records) queues the append pass into a buffer of cap_records
 *   records behind one counter; _window_fetch copies counter and records in one transfer, *out_n = records stored; more matches than
 *   cap_records are never written and reported as SPHX_ERR_CAPACITY.  Record: {id - first_id, slot, x, y, vx, vy, density, 0}.
 *   _record / _frame / _read are the recorder's seam; a frame of _read is [unique] x 16 bytes, then [unique] presence words.
 * Cost: per tile 4 bytes per local particle scanned, 24 bytes per distinct id (fetch) or 32 per owned particle of the window back to the
 *   host; DESIGN.md section 4m. */
typedef struct sphx_multi_track_out {
    uint32_t* tile;    /* [m] global tile rank that owns the id, or SPHX_TRACK_ABSENT; or NULL */
    uint32_t* slot;    /* [m] index in that tile's sphx_download order, or SPHX_TRACK_ABSENT; or NULL */
    float* pos;        /* [2m] or NULL */
    float* vel;        /* [2m] or NULL */
    float* density;    /* [m] or NULL */
} sphx_multi_track_out;   /* host pointers; not all NULL */
int sphx_multi_track_set(sphx_multi* m, const uint32_t* ids /* host */, uint32_t n_ids);
int sphx_multi_track_fetch(sphx_multi* m, uint32_t flags /* 0 */, const sphx_multi_track_out* out);
int sphx_multi_track_record(sphx_multi* m, uint32_t max_frames, uint32_t every);
int sphx_multi_track_get_status(const sphx_multi* m, sphx_track_status* out);
int sphx_multi_track_read(sphx_multi* m, uint32_t first_frame, uint32_t n_frames, uint32_t flags /* 0 */,
                          float* out /* [n_frames][m][4] */, uint32_t* out_tile /* [n_frames][m], may be NULL */);
int sphx_multi_download_by_id(sphx_multi* m, uint32_t first_id, uint32_t count, uint32_t flags /* 0 */,
                              const sphx_multi_track_out* out, uint32_t* out_present /* may be NULL */);
int sphx_track_merge(uint32_t m, const sphx_multi_track_out* parts, uint32_t n_parts, const sphx_multi_track_out* out, uint32_t* out_present /* may be NULL */);
int sphx_track_merge_frames(uint64_t n /* n_frames * m */, const float* const* parts /* [n_parts] of [n][4] */, const uint32_t* const* parts_tile /* [n_parts] of [n] */,
                            uint32_t n_parts, float* out /* [n][4] */, uint32_t* out_tile /* [n], may be NULL */);
int sphx_tile_track_install(sphx_ctx* tile_ctx, const uint32_t* table /* host, [unique] ascending */, const uint32_t* filter /* host, 2^log2_bits bits */,
                            uint32_t unique, uint32_t log2_bits);
int sphx_tile_track_fetch_enqueue(sphx_ctx* tile_ctx);
int sphx_tile_track_fetch(sphx_ctx* tile_ctx, uint32_t* slot /* host, [unique] */, float* xyvv /* host, [unique][4] */, float* density /* host, [unique] */);
int sphx_tile_track_window_enqueue(sphx_ctx* tile_ctx, uint32_t first_id, uint32_t count, uint32_t cap_records);
int sphx_tile_track_window_fetch(sphx_ctx* tile_ctx, uint32_t* records /* host, [4 + 8 * cap_records]: the counter's 16 bytes, then the records */,
                                 uint32_t* out_n);
int sphx_tile_track_record(sphx_ctx* tile_ctx, uint32_t max_frames, uint32_t every);
int sphx_tile_track_frame(sphx_ctx* tile_ctx); /* one finished step: a frame if the recording is due */
int sphx_tile_track_read(sphx_ctx* tile_ctx, uint32_t first_frame, uint32_t n_frames, float* xyvv /* host, [n_frames][unique][4] */,
                         uint32_t* slot /* host, [n_frames][unique] */);
/* ---- sampling the fields of a tiled run (csrc/sphx_tiles.cpp; device passes csrc/sphx_sample.inc, lattice windows and the fold
 * csrc/sphx_sample_window.hpp) ---------------------------------------------------------------------------------------------------------
 * sphx_sample_points / sphx_sample_grid for a sphx_multi, without sphx_multi_download and a second context.
 * Who answers: the tile whose owned cell rectangle contains cell_of(q) — the grid's fp32 cell function of "field sampling" above
 *   (saturating, a NaN coordinate goes to cell 0).  The rectangles of a layout partition [0, 65536)^2 ("picture of a tiled run"), so every
 *   point has exactly one answering tile.
 * What it computes: the contract of sphx_sample_points, word for word, over THAT TILE'S OWN ARRAYS — candidates, acceptance, kernels,
 *   summation order and outputs; "device index" is the tile's local index (the order of sphx_download on sphx_multi_tile_ctx, ghosts
 *   included), "boundary" the tile's clipped boundary set (sphx_download_boundary on it).  One device function walks a point in all
 *   four calls.  Consequences: (a) the result is bit-identical to the restatement of that contract over the answering tile's own
 *   downloads, in every mode; (b) in tiling-invariant mode (sphx_set_tiling_invariant: cell mates ordered by id in a tile and in a single
 *   context alike; a clipped boundary keeps the caller's order) it is bit-identical to sphx_sample_points of a single context in the
 *   same mode; (c) the lattice call is bit-identical to the points call at the same fp32 points.
 * The ghost band: a point in an owned cell walks the 3 x 3 cells around it and, across a cut, reads position, velocity and density of
 *   ring-1 ghosts.  Positions of ghosts are exact after every exchange (they only change with the advection that rides on one);
 *   velocities are exact in `valid` rings, densities in `avalid` rings (the tile loop's ring budget: a halo exchange sets valid = kvalid =
 *   halo and avalid = halo - 1, a warm start costs valid a ring, every solver iteration two).  valid >= 1 and avalid >= 1 therefore mean
 *   "ring-1 ghosts hold final position, velocity and density", and need(min(avalid, valid) - 1) — the very test the next
 *   sphx_multi_step_begin makes before its non-pressure pass — is the precondition of a query.  Both calls make it before any tile
 *   enqueues:
 *     a ring is left: nothing is exchanged, the call only reads (a queued run-ahead pass stays valid, the sweep direction is put back);
 *     the band is spent: the halo exchange and re-grid the next step_begin owes happen NOW instead of then — the plain exchange of
 *       the tile loop on the same state (after a finished step no advection is pending: the step's own exchange has applied it), so the
 *       run is unchanged.  In this case alone sphx_multi_info().exchanges moves one earlier; after the next sphx_multi_step_begin the
 *       count is the same either way.
 *   Because of that exchange the calls are COLLECTIVE in rank mode: every rank calls at the same point of the run with the same points.
 * In-process (sphx_multi_create): every point is answered; out->tile is optional.  Rank mode (sphx_multi_create_rank): the call fills
 *   the points this rank's tile answers; every other entry of every requested array is written as zero with tile = -1, and out->tile is
 *   required.  The caller moves the parts with its own transport and folds them with sphx_sample_merge(m, parts, n_parts, out): pure host
 *   code; per point the part with tile >= 0, the lowest tile if several have one, zeros and -1 if none; every part carries tile and the
 *   arrays out asks for (SPHX_ERR_INVALID_ARGUMENT otherwise); n_parts == 0 gives the all-absent answer; out may alias parts[0].
 * A tile without any particle (it owns cells, perhaps walls, and no fluid) answers from its static grid alone: the density next to a wall
 *   there equals the single context's.
 * When allowed: after sphx_multi_upload (its warm-up block ends with the re-grid that computes the densities of the uploaded positions,
 *   on owned particles and ghosts alike: density_valid of sphx_multi_fluid_stats) and after every finished step.  SPHX_ERR_NOT_READY
 *   between sphx_multi_step_begin and _finish, before the first upload, on a multi a failed sphx_multi_state_load left broken and on one
 *   whose collective step has failed.  SPHX_ERR_INVALID_ARGUMENT (sphx_multi_last_error names the argument): m, out NULL, xy NULL with
 *   n > 0, n >= 2^31, out requesting none of the four fields, an unknown kernel_kind, any flags bit (there is no device-pointer path
 *   across several devices), the lattice errors of sphx_sample_grid, more than 64 tiles, rank mode without out->tile.  n == 0 and
 *   nx * ny == 0 are successful no-ops once the arguments pass.  A refused call touches no tile.
 * Device work per tile.  Points: all n points go up (8 bytes each); a selection pass appends the indices of the points the tile owns to
 *   a list (one atomic per wavefront), the walk runs over that list with every lane live and writes one packed 24-byte record {index,
 *   density, fraction, vx, vy, count} per answered point; only those records come back and the host scatters them by index.  Lattice:
 *   the points a tile owns form an index rectangle (the cell of x0 + (float)ix * dx is monotone in ix), found on the host by bisection
 *   over the exact fp32 expression; the tile walks that window alone, the host copies its rows into the full arrays.  The points
 *   the K tiles walk together are those of one query, not of K; their launches add up (every tile also reads all n points in its
 *   selection pass), so the summed device time of a small query grows with K.  Figures: DESIGN.md section 4n.
 * Inspection: sphx_multi_tile_rects writes the owned rectangles of ALL world tiles in rank order (*inout_n: capacity in, world out;
 *   SPHX_ERR_CAPACITY if it was smaller, SPHX_ERR_NOT_READY before the first upload); sphx_multi_ghost_rings writes {valid, kvalid,
 *   avalid} of local tile 0 (+INFINITY on a one-tile run).
 * One tile (INTERNAL, like the other sphx_tile_* calls; accepted only on a tile context — sphx_sample_* keep refusing one):
 *   sphx_tile_sample_points enqueues upload, selection and walk for the fields named by SPHX_SAMPLE_FIELD_* bits, _points_fetch copies
 *   back *out_n records of six words (more than cap_records: SPHX_ERR_CAPACITY); sphx_tile_sample_window enqueues the walk over the
 *   tile's window of the lattice and reports it as out_window = {ix0, ix1, iy0, iy1} (all zero: the tile owns no lattice point),
 *   _window_fetch copies the window-sized arrays back, row after row (out names exactly the queued fields).  SPHX_ERR_NOT_READY between
 *   a halo exchange and the tile's re-grid. */
enum { SPHX_SAMPLE_FIELD_DENSITY = 1u, SPHX_SAMPLE_FIELD_FRACTION = 2u, SPHX_SAMPLE_FIELD_VELOCITY = 4u, SPHX_SAMPLE_FIELD_COUNT = 8u };
typedef struct sphx_multi_sample_out {   /* host arrays; any non-empty subset of the first four */
    float* density;    /* [m] or NULL */
    float* fraction;   /* [m] or NULL */
    float* velocity;   /* [2m] interleaved xy, or NULL */
    uint32_t* count;   /* [m] or NULL */
    int32_t* tile;     /* [m] or NULL: global rank of the tile that answered, -1: none of the local tiles */
} sphx_multi_sample_out;
int sphx_multi_sample_points(sphx_multi* m, const float* xy /* host */, uint32_t n, int kernel_kind, uint32_t flags /* 0 */, const sphx_multi_sample_out* out);
int sphx_multi_sample_grid(sphx_multi* m, float x0, float y0, float dx, float dy, uint32_t nx, uint32_t ny, int kernel_kind, uint32_t flags /* 0 */,
                           const sphx_multi_sample_out* out);
int sphx_sample_merge(uint32_t m, const sphx_multi_sample_out* parts, uint32_t n_parts, const sphx_multi_sample_out* out);
int sphx_multi_tile_rects(const sphx_multi* m, sphx_tile_rect* out /* [*inout_n] */, uint32_t* inout_n);
int sphx_multi_ghost_rings(const sphx_multi* m, double* out3);
int sphx_tile_sample_points(sphx_ctx* tile_ctx, const float* xy /* host, [2m] */, uint32_t m, int kernel_kind, uint32_t fields);
int sphx_tile_sample_points_fetch(sphx_ctx* tile_ctx, uint32_t* records /* host, [6 * cap_records] */, uint32_t cap_records, uint32_t* out_n);
int sphx_tile_sample_window(sphx_ctx* tile_ctx, float x0, float y0, float dx, float dy, uint32_t nx, uint32_t ny, int kernel_kind, uint32_t fields,
                            uint32_t* out_window /* [4] */);
int sphx_tile_sample_window_fetch(sphx_ctx* tile_ctx, const sphx_sample_out* out /* host, window-sized */);

/* ---- free surface of a tiled run (csrc/sphx_tiles.cpp; device passes csrc/sphx_contour.inc and csrc/sphx_sample.inc, apron look-up and
 * merge csrc/sphx_contour_merge.hpp) ---------------------------------------------------------------------------
 * sphx_surface_contour for a sphx_multi, without sphx_multi_download and a second context and without the lattice crossing to the host.
 * Lattice values: node (ix, iy) has the value sphx_multi_sample_grid returns for the chosen field at that lattice, kernel and state: the
 *   tile that owns the node's grid cell answers it over its own arrays, with the one device function.  Consequences (a) to (c) of
 *   "sampling the fields of a tiled run" carry over.  There is no `values` output: sphx_multi_sample_grid returns those bits.
 * Who cuts a cell: lattice cell (ix, iy) is cut by the tile whose window (csrc/sphx_sample_window.hpp) holds its node 0 = (ix, iy).  The
 *   windows partition the lattice, so every cell is cut exactly once.  The other three nodes may be another tile's: a tile samples its
 *   window into an array padded by one apron column and row, and the tiles swap the first row and first column of their windows (every
 *   apron node is in one of those) as bit patterns through the host.  A node that no border holds is SPHX_ERR_HIP, never a zero.
 * Marching squares: the inside test, cases, saddle rule, edge naming, crossing point, segment direction and the order inside a cell are
 *   those of "free-surface extraction" above, word for word, evaluated with GLOBAL lattice indices: the point is x0 + (float)ix*dx, never
 *   a shifted origin, and the cell word is iy*(nx-1)+ix.
 * In-process (sphx_multi_create): *count is the total over all tiles; the output is in ascending global cell index, within a cell as
 *   above.  In tiling-invariant mode that is byte for byte the output of sphx_surface_contour on a single context in the same mode; in
 *   every mode it is byte for byte the contract applied to the values of sphx_multi_sample_grid on the same state.  Capacity as in the
 *   single call: the first cap_segments segments of the global order are written, nothing at or behind the capacity is written.  Each
 *   tile is asked for min(cap_segments, 2 * its cells) segments, which suffices: a segment among the first cap_segments of the global
 *   order is among the first cap_segments of its tile.  out->tile[k] is the tile that cut the cell of segment k.
 * Rank mode (sphx_multi_create_rank): the call returns this rank's part — the count of its tile and its first min(count, cap_segments)
 *   segments in its own ascending cell order; out->cell is required whenever cap_segments > 0.  The borders cross the ranks in one vector
 *   of known layout, each rank filling its own entries as (double)(uint32 bit pattern) and zeros elsewhere, summed by the all-reduce of
 *   sphx_comm_ops eight words at a time (integers below 2^32: exact); the exchange op is not used.  The caller moves the parts and folds
 *   them with sphx_contour_merge: pure host code, a stable K-way merge by cell word (of equal words the earlier part first, within a part
 *   the stored order).  stored[p] is how many entries part p holds; *out->count becomes the sum of the parts' counts.  If any part has
 *   count > stored the merge sets the count, writes no segment and returns SPHX_ERR_CAPACITY — the caller then knows what capacity to
 *   retry with.  Otherwise it writes the first cap_segments of the merged order; n_parts == 0 gives count 0.  out may alias no part.
 * When allowed, refusals, side effects: as sphx_multi_sample_grid — the same SPHX_ERR_NOT_READY rules, lattice errors and 64-tile
 *   limit, the same ghost-band precondition and "exchange now instead of at the next step_begin" behaviour, so the call is COLLECTIVE
 *   in rank mode; a run with calls between its steps is bit-identical to one without.  Further SPHX_ERR_INVALID_ARGUMENT: iso not
 *   finite, an unknown field or kernel_kind, any flags bit, out or out->count NULL, rank mode with cap_segments > 0 and out->cell NULL.
 *   nx < 2, ny < 2 or nx*ny == 0 is a successful call with count 0.  A refused call touches no tile; the argument checks come before
 *   the band exchange.
 * One tile (INTERNAL, like the other sphx_tile_* calls; accepted only on a tile context): sphx_tile_contour_sample enqueues the walk over
 *   the tile's window into the padded array and the border pack, and reports the window {ix0, ix1, iy0, iy1} (all zero: the tile owns no
 *   node); _border_fetch copies the window's row 0 and column 0 back (w + h words); _cut takes the apron (last column rows [iy0, iy1) if
 *   ix1 < nx, then last row columns [ix0, ix1) if iy1 < ny, then the corner if both), uploads and unpacks it and enqueues count, carry and
 *   emit for min(cap_segments, 2 * cells) segments; _fetch copies back the count, then min(count, cap) segments and cell words.  The
 *   scratch grows on demand on the tile's context and is freed in sphx_destroy; no atomics, the sweep direction is put back. */
typedef struct sphx_multi_contour_out {   /* host arrays */
    float*    segments;  /* [cap_segments][4] or NULL */
    uint32_t* cell;      /* [cap_segments] GLOBAL cell index iy*(nx-1)+ix, or NULL (required in rank mode) */
    int32_t*  tile;      /* [cap_segments] global rank of the tile that emitted the segment, or NULL */
    uint32_t* count;     /* [1] required */
} sphx_multi_contour_out;
int sphx_multi_surface_contour(sphx_multi* m, float x0, float y0, float dx, float dy, uint32_t nx, uint32_t ny, int kernel_kind,
                               int field, float iso, uint32_t cap_segments, uint32_t flags /* 0 */, const sphx_multi_contour_out* out);
int sphx_contour_merge(const sphx_multi_contour_out* parts, const uint32_t* stored /* [n_parts] */, uint32_t n_parts,
                       uint32_t cap_segments, const sphx_multi_contour_out* out);
int sphx_tile_contour_sample(sphx_ctx* tile_ctx, float x0, float y0, float dx, float dy, uint32_t nx, uint32_t ny, int kernel_kind, int field,
                             uint32_t* out_window /* [4] */);
int sphx_tile_contour_border_fetch(sphx_ctx* tile_ctx, uint32_t* border /* host, [cap_words] */, uint32_t cap_words);
int sphx_tile_contour_cut(sphx_ctx* tile_ctx, float iso, uint32_t cap_segments, const uint32_t* apron /* host, [n_apron] */, uint32_t n_apron);
int sphx_tile_contour_fetch(sphx_ctx* tile_ctx, float* segments /* host or NULL */, uint32_t* cell /* host or NULL */, uint32_t* out_count);

/* ---- per-particle flow fields of a tiled run (csrc/sphx_fields.inc, csrc/sphx_tiles.cpp) --------------------------------
 * sphx_particle_fields for a sphx_multi: velocity gradient, divergence, vorticity and colour-field gradient at every particle the local
 * tiles own, without a download and a second context.  A tile holds what the query needs: an owned particle's neighbour list is complete,
 * and the ghost band carries its neighbours' position, velocity and density.
 * What it computes: for every particle a local tile owns (bit 31 of its id word) the contract of sphx_particle_fields applies word for
 *   word, evaluated over THAT TILE'S OWN ARRAYS, ghosts included: the list is the one sphx_download_neighbors on sphx_multi_tile_ctx
 *   returns for the particle, positions, velocities and densities are the bits sphx_download on that tile context returns, "boundary"
 *   means the tile's clipped boundary set; the fp32 order of operations is unchanged and a capped list stays capped.  A ghost is never
 *   answered and never written (its list is not complete).  Any subset of the outputs gives the same bits as the full set.
 * Order of the output: that of sphx_multi_download — the local tiles in order, within a tile the owned particles in the tile's device
 *   order.  *inout_n: capacity in (entries), count out.  Entry k lines up with entry k of a sphx_multi_download made AFTER the call and
 *   before the next step — not with one made before it, because the call may re-grid (the ghost band, below).  out->ids (the particle id
 *   of entry k, 31 bits) is always the safe key; out->tile is the global rank of the tile that owns entry k.
 * Consequences: (a) in every mode the result is bit-identical to tests/fields_reference.py::fields32 over the answering tile's own
 *   downloads; (b) in tiling-invariant mode (sphx_set_tiling_invariant) it is bit-identical to sphx_particle_fields of a single context
 *   in the same mode, matched by id.
 * The ghost band: the precondition of tiled sampling (above) — ring-1 ghosts must hold final position, velocity and density, i.e.
 *   need(min(avalid, valid) - 1), tested before any tile enqueues.  A ring is left: the call only reads (the sweep direction is put back,
 *   a queued run-ahead pass stays valid).  The band is spent: the halo exchange and re-grid the next sphx_multi_step_begin owes happen
 *   NOW; in this case alone sphx_multi_info().exchanges moves one earlier.  Because of that exchange the call is COLLECTIVE in rank mode.
 *   A run with calls between its steps is bit-identical to one without: every sphx_step_stats field, every sphx_multi_state_digest word,
 *   the rebalances.
 * When allowed: after sphx_multi_upload (its warm-up block leaves lists and densities for the uploaded positions), after
 *   sphx_multi_state_load, after every finished step, after sphx_multi_append / _remove (they end in a re-grid).  SPHX_ERR_NOT_READY
 *   before the first upload, between sphx_multi_step_begin and _finish, on a multi a failed sphx_multi_state_load left broken and on one
 *   whose collective step has failed.  SPHX_ERR_INVALID_ARGUMENT (sphx_multi_last_error names the argument): m, out or inout_n NULL, all
 *   four field pointers NULL, any flags bit (there is no device-pointer path across several devices).  SPHX_ERR_CAPACITY: *inout_n is
 *   smaller than the owned count of the local tiles; *inout_n receives that count and no output is written — the test comes after the
 *   band check and before any walk (each tile counts its owned particles on its device: 4 bytes per local particle).  A refused call
 *   touches no tile.  Zero owned particles is a successful no-op with *inout_n = 0.
 * Rank mode (sphx_multi_create_rank): each rank returns its own tile's part; the whole answer is the parts concatenated in rank order.
 *   No merge function is needed: no particle has two owners.
 * Device work per tile: a counting pass over the id words (owned lanes per wavefront and per 256-slot piece), the exclusive scan of the
 *   pieces, and the walk of sphx_particle_fields in its owned-only form — a piece without an owned particle leaves at once, a ghost
 *   stages and walks nothing, an owned particle writes at its place among the owned ones (no atomic: two calls give the same bytes in
 *   the same places).  Only the owned entries come back.
 * One tile (INTERNAL, like the other sphx_tile_* calls; accepted only on a tile context): sphx_tile_owned_count runs count + scan and
 *   returns the owned count; sphx_tile_particle_fields_enqueue queues count, scan and walk for the fields named by SPHX_FIELD_* bits into
 *   a scratch of the tile (grown on demand, freed in sphx_destroy; want_ids: the ids too), _fetch copies back *out_n owned entries (out
 *   names exactly the queued fields; more than cap: SPHX_ERR_CAPACITY with *out_n set).  SPHX_ERR_NOT_READY between a halo exchange and
 *   the tile's re-grid. */
enum { SPHX_FIELD_VEL_GRAD = 1u, SPHX_FIELD_DIVERGENCE = 2u, SPHX_FIELD_VORTICITY = 4u, SPHX_FIELD_COLOR_GRAD = 8u };
typedef struct sphx_multi_fields_out {   /* host arrays */
    float* vel_grad;    /* [4n] or NULL */
    float* divergence;  /* [n]  or NULL */
    float* vorticity;   /* [n]  or NULL */
    float* color_grad;  /* [2n] or NULL */      /* not all four NULL */
    uint32_t* ids;      /* [n] or NULL: particle id of entry k (31 bits) */
    int32_t* tile;      /* [n] or NULL: global rank of the tile that owns entry k */
} sphx_multi_fields_out;
int sphx_multi_particle_fields(sphx_multi* m, uint32_t flags /* 0 */, const sphx_multi_fields_out* out, uint64_t* inout_n);
int sphx_tile_owned_count(sphx_ctx* tile_ctx, uint32_t* out_owned);
int sphx_tile_particle_fields_enqueue(sphx_ctx* tile_ctx, uint32_t field_mask, uint32_t want_ids);
int sphx_tile_particle_fields_fetch(sphx_ctx* tile_ctx, const sphx_fields_out* out /* host */, uint32_t* ids /* host or NULL */, uint32_t cap, uint32_t* out_n);
/* Solver::simulation_step(&mut world, &mut time_manager) (solver/mod.rs:17) in ONE call: phase A, the TimeManager mirror
 * (simulation_step() dfsph.rs:433, update_simulation_step dfsph.rs:478-480), phase B */
struct sphx_timer;
int sphx_multi_simulation_step(sphx_multi* m, struct sphx_timer* timer, float particle_diameter, sphx_step_stats* out_stats);
/* `k` of those back to back — the caller's frame loop (main.rs:348-350 -> single_sim_step, :279) on this side of the boundary, for
 * hosts whose per-call cost matters (a Python driver).  out_stats: k entries or NULL; *out_done (may be NULL) = steps finished;
 * stops at the first failing step and returns its code. */
int sphx_multi_simulation_steps(sphx_multi* m, struct sphx_timer* timer, float particle_diameter, uint32_t k, sphx_step_stats* out_stats,
                                uint32_t* out_done);

/* ---- picture of a tiled run (csrc/sphx_render.inc, csrc/sphx_render_window.hpp, csrc/sphx_render_merge.hpp, csrc/sphx_tiles.cpp) ---------------
 * sphx_render's picture (above: pixel geometry, coverage test, disc radius, colour formula, argument errors and limits) of a run that is
 * cut into tiles, without a sphx_multi_download: 4 bytes per pixel come back instead of 24 per particle.  The calls read only pos, vel and
 * particle_id of the particles each tile OWNS (bit 31 of the id in the tile's arrays) and the tile's boundary particles; these are exact
 * after every finished step whatever the ghost band has spent, so no halo exchange is made.
 * The owner of a pixel — sphx_render's is "the highest device index among all covering fluid particles", and a tiled run has no global
 * index.  It needs none: inside a tile the owned particles stand in the order a single context would hold them in (ascending Morton
 * code of the cell, cell mates in their relative order); every cell belongs to exactly one tile (the tiles' rectangles partition
 * [0, 65536)^2); so of two covering particles of different tiles the one whose cell has the greater Morton code comes later in a single
 * context's array.  The COMPOSITE RULE:
 *   per tile     the owner is the highest local index among the covering fluid particles the tile owns;
 *   across tiles the owner whose cell has the greater Morton code wins: cell = position_to_mortoncellpos(x_owner)
 *                (neighborhood_search.rs:52-58, the grid's fp32 cell function), code = morton.rs' encode of it;
 *   fluid beats boundary, boundary beats background.
 * A LAYER (sphx_render_layer) is one tile's — or several tiles' merged — picture at the full size of the view: per pixel `owner` = the
 * particle ID (< 2^31; not an index: a tile's indices mean nothing outside it) of a fluid owner, SPHX_RENDER_BOUNDARY or SPHX_RENDER_NONE,
 * `key` = the Morton code of the fluid owner's cell, else 0, and `rgba` = sphx_render's bytes for that owner (background for NONE).
 * A tile's layer shows the fluid particles it owns and the boundary particles it holds whose cell lies in its rectangle (the tiles'
 * clipped boundary sets contain those; together they are the whole boundary).
 * sphx_render_merge(width, height, layers, n_layers, out): pure host code, no context, no GPU.  Folds the layers in the order given: per
 *   pixel the class is fluid (2), boundary (1) or none (0); a later layer replaces what has accumulated only if its class is higher, or
 *   if both are fluid and its key is STRICTLY greater (equal keys — impossible between tiles of one run — keep the earlier layer).  key,
 *   owner and rgba travel together: no byte of a losing layer reaches the result.  Every non-NULL array of out is written; out may alias
 *   layers[0].  SPHX_ERR_INVALID_ARGUMENT: out NULL or all three of its arrays NULL, layers NULL with n_layers > 0, a layer without key or
 *   owner, out->rgba requested and a layer without rgba, width * height >= 2^28, n_layers == 0 with out->rgba requested (no layer supplies
 *   the background colour; without rgba n_layers == 0 fills the picture with NONE).
 * sphx_multi_render(m, view, flags = 0, out): the whole run's picture, out->rgba and / or out->owner (host) as sphx_render fills them but
 *   for the owners, which are particle IDs (and the two codes).  Every local tile enqueues its layer on its own stream and device; the
 *   layers are copied back and merged in ascending tile rank.  In-process only (sphx_multi_create): in rank mode it returns
 *   SPHX_ERR_INVALID_ARGUMENT — there each rank takes sphx_multi_render_layer, the caller moves the layers with its own transport and
 *   merges them with sphx_render_merge.  With one tile the picture equals sphx_render's of that particle set, ids for indices.
 * sphx_multi_render_layer(m, view, flags = 0, out): the merged layer of the LOCAL tiles (in-process: all; rank mode: this rank's one);
 *   any non-empty subset of out's arrays (host).  No communication: not collective, a rank may call it alone.
 * The window: a tile clears, scatters into, resolves and copies back only the pixel rectangle its owned cells can reach (its cell
 *   rectangle in world units grown by the disc radius and a margin, converted conservatively to pixels, clipped to the image; an edge at
 *   cell 0 or 65536 extends to the image's edge: the saturated cells hold particles from anywhere beyond the domain).  K tiles cost about
 *   one frame plus the seams, not K frames.
 * When allowed: wherever sphx_multi_download is — after sphx_multi_upload and after every finished step.  SPHX_ERR_NOT_READY between
 *   sphx_multi_step_begin and _finish, before the first sphx_multi_upload, and on a multi a failed sphx_multi_state_load left broken.
 *   SPHX_ERR_INVALID_ARGUMENT: m / view / out NULL, out requesting nothing, any flags bit, the view errors of sphx_render (same messages),
 *   more than 64 tiles.  width * height == 0 is a successful no-op.
 * One tile (INTERNAL, like the other sphx_tile_* calls): sphx_tile_render_layer is accepted ONLY on a tile context (a plain one:
 *   SPHX_ERR_INVALID_ARGUMENT; sphx_render keeps refusing a tile context), takes SPHX_RENDER_DEVICE_POINTERS like sphx_render (full-size
 *   device arrays, enqueued, not waited for) and returns SPHX_ERR_NOT_READY between a halo exchange and the tile's re-grid.
 *   sphx_tile_render_window is the first half of the multi's call: the tile's passes are enqueued, out_window = {x0, x1, y0, y1} (pixel
 *   columns and rows, all zero: nothing to fetch) and out_dev = device arrays holding the WINDOW's pixels only, row after row, valid until
 *   the context renders again; nothing is waited for.
 * No side effects: all of this only reads (a queued run-ahead pass stays valid, the sweep direction is put back).  A run with these calls
 *   between its steps is bit-identical to the same run without: everything sphx_multi_download returns, every sphx_step_stats field,
 *   sphx_multi_info().exchanges.
 * Cost: DESIGN.md section 4k. */
typedef struct sphx_render_layer {   /* one tile's (or one rank's) picture of the particles it owns, full view size */
    uint32_t* key;    /* [height*width]: morton(cell_of(x_owner)) for a fluid owner, else 0 */
    uint32_t* owner;  /* [height*width]: particle id (< 2^31) of a fluid owner, SPHX_RENDER_BOUNDARY, or SPHX_RENDER_NONE */
    uint8_t*  rgba;   /* [height*width*4] or NULL */
} sphx_render_layer;
int sphx_multi_render(sphx_multi* m, const sphx_render_view* view, uint32_t flags /* 0 */, const sphx_render_out* out /* host */);
int sphx_multi_render_layer(sphx_multi* m, const sphx_render_view* view, uint32_t flags /* 0 */, const sphx_render_layer* out /* host */);
int sphx_render_merge(uint32_t width, uint32_t height, const sphx_render_layer* layers, uint32_t n_layers, const sphx_render_layer* out);
int sphx_tile_render_layer(sphx_ctx* tile_ctx, const sphx_render_view* view, uint32_t flags, const sphx_render_layer* out); /* INTERNAL seam */
int sphx_tile_render_window(sphx_ctx* tile_ctx, const sphx_render_view* view, uint32_t want_rgba, uint32_t* out_window /* [4] */,
                            sphx_render_layer* out_dev); /* INTERNAL seam */

/* ---- checkpoint of a tiled run (csrc/sphx_multi_state.inc, csrc/sphx_multi_state_format.hpp, csrc/sphx_tiles.cpp) ---------------------------
 * A sphx_multi put down and picked up, without sphx_multi_download (which drops the warm-start sums that travel with the particles in tile
 * mode and the iteration counts that decide whether the warm starts fire) and without the warm-up block of sphx_multi_upload.  The
 * checkpoint is taken on the device from the particles each tile OWNS (bit 31 of the id in the tile's arrays) and is tiling-independent in
 * content: what 2 x 2 tiles saved loads into 2 strips, 8 strips or one tile.
 * Parts: a checkpoint is n_parts blobs.  An in-process sphx_multi (sphx_multi_create) writes ONE part, "part 0 of 1", its tiles in ascending
 *   rank; in rank mode (sphx_multi_create_rank) every rank writes its own part "r of W" and nothing crosses the ranks for a save.  A part
 *   (byte-exact layout: the top of csrc/sphx_multi_state_format.hpp), little-endian: magic "SPHXMULT" (not the single-context blob's),
 *   version, endianness tag, total size; the sphx_params with device stored as 0; N_total, N_part, B, part, n_parts; num_density_iters,
 *   num_divergence_iters, last_div_iters, last_div_warm, steps; the tiling-invariant flag; the saver's layout (world, axis / nx / ny, the
 *   cuts in a fixed-size array for <= 64 tiles); a table of {offset, bytes, digest} and a digest of the header; then SPHX_MULTI_STATE_SECTIONS
 *   sections, 8-byte aligned, padding zero: positions, velocities, particle_id (bit 31 cleared), density, alpha, kappa, stiffness of the
 *   part's particles in the tiles' device order, and the GLOBAL boundary in caller order.  No timestamp, no pointer: two saves of one state
 *   are byte-identical.
 * Digest of a particle section with k 32-bit words per particle, all arithmetic mod 2^64 — the section digest above with the word index
 *   replaced by id * k + c:
 *     D = sum_owned sum_{c<k} (uint64)w[c] * ((2 (id k + c) + 1) * 0x9E3779B97F4A7C15)  +  (n_owned k) * 0xD6E8FEB86659FD93
 *   For ids 0 .. N-1 it equals the section digest of the id-ordered array (sphx_download_by_id).  Integer arithmetic: it depends neither
 *   on the order of accumulation nor on the tiling, and the digest of the whole run is the plain sum of the tiles' (and of the parts').
 *   The boundary section carries the positional digest.  NOT a cryptographic hash, as above.
 * Canonical warm-start values: with num_density_iters <= 1 the kappa section is written, and digested, as +0.0 (the next density loop
 *   zeroes kappa before it reads it, dfsph.rs:199, and the tile loop did not even move it); the same for stiffness with
 *   num_divergence_iters <= 1 (dfsph.rs:354).
 * sphx_multi_state_size / _save(buf: host, flags = 0): every local tile enqueues its pass on its own stream and device — three launches,
 *   36 bytes read per local particle (+ 4 for the count), 36 written per owned one — then copies its sections into buf at its offsets.
 *   A capacity below the size: SPHX_ERR_CAPACITY with the needed size in *out_bytes (may be NULL).
 * sphx_multi_state_digest: out[0 .. 7) the id-keyed digests of the WHOLE run's live particle sections, out[7] the boundary's.  Rank mode:
 *   COLLECTIVE; the 64-bit sums cross the ranks as integers below 2^32 and every rank receives the same 64 bytes.
 * sphx_multi_state_load(parts, bytes, n_parts, flags = 0) follows sphx_multi_upload's path; every rank is given ALL parts (collective), as
 *   every rank is given the global arrays there.  Host validation first — per part: magic, version, endianness, sizes, section bounds and
 *   overlaps, every count against every other, ids below 2^31, zero padding, the boundary's digest; the set: every part index once, scalars,
 *   params, flag, layout and boundary equal across the parts, sum of N_part = N_total; the params against the multi's by sphx_state_load's
 *   rule (every field except device and list_span_limit bit for bit; the message names the first that differs); a checkpoint saved in
 *   tiling-invariant mode loads only into a multi whose tiles are in that mode and the other way round.  A refusal at this stage is
 *   SPHX_ERR_INVALID_ARGUMENT and leaves the multi UNTOUCHED.  No count is used before it has been checked.  Then: the layout is an
 *   explicit sphx_multi_set_layout / _set_grid_layout, else the saved cuts if the saver had as many tiles as this multi, else the
 *   quantile layout of sphx_multi_upload over the checkpoint's positions; the boundary becomes the checkpoint's; every tile keeps its
 *   rectangle's particles WITH their warm-start values (sphx_tile_upload_state); the iteration counts, last_div_* and steps are restored;
 *   the ring budget of the ghost band and the info counters start as after an upload.  ONE halo exchange and re-grid runs (ghosts,
 *   neighbour lists, densities and alpha recomputed): not the warm-up block — the counts are kept — and no SPHX_FLAG_* is raised.  Each
 *   tile then digests what it owns: the sums for positions, velocities, particle_id, kappa and stiffness must equal the parts'; otherwise
 *   SPHX_ERR_INVALID_ARGUMENT naming the section, and the multi asks for an upload or a load (steps, statistics and saves return
 *   SPHX_ERR_NOT_READY).  A statistics recording survives, as it does over an upload.
 * When allowed: save, size and digest wherever sphx_multi_fluid_stats is; SPHX_ERR_NOT_READY before the first upload or load, between
 *   sphx_multi_step_begin and _finish and on a multi a failed collective step has poisoned; load is allowed before the first upload too.
 *   Any flags bit, NULL arguments, more than 64 tiles: SPHX_ERR_INVALID_ARGUMENT.
 * Files: sphx_multi_state_save_file writes the part to path (in-process) or to path + ".rRRRofWWW" (rank mode: three decimal digits each,
 *   e.g. ".r001of004"), to a ".tmp" name renamed when complete.  sphx_multi_state_load_file reads `path` if it exists (one or several parts
 *   back to back), else the complete set path.r000ofWWW ...; an incomplete set or an I/O failure is SPHX_ERR_INVALID_ARGUMENT.
 * THE PROMISE.
 *   1. In any mode, directly after a load the run holds exactly the saved particles: positions, velocities, ids, kappa and stiffness bit
 *      for bit by id, and the counts behind the warm starts.  Two multis that load the same parts with the same world and layout then
 *      produce identical bits.
 *   2. In tiling-invariant mode (sphx_set_tiling_invariant on every tile) with fixed iteration counts the loaded run continues
 *      bit-identically by id to the run that saved, for any tiling of the loader including one tile, and after the load all eight digests
 *      equal the checkpoint's.
 *   3. In default mode a continued run is a valid run of the same state, not a bit-equal one: the load re-decomposes and re-exchanges,
 *      which is the sense in which two tilings of one scene differ (DESIGN.md section 4j has the measured spread).
 * No side effects of save, size and digest: they only read the tiles' state (a queued run-ahead pass stays valid, the sweep direction is put
 *   back); a run with saves and digests between its steps is bit-identical to the same run without.
 * One tile (INTERNAL, like the other sphx_tile_* calls): sphx_tile_state_pack enqueues the pass on a tile context and hands out the seven
 *   DEVICE section buffers (the context's own scratch, valid until the next pack or upload); with out_digests or out_n_owned non-NULL it
 *   then waits and returns them, otherwise sphx_tile_state_fetch does later (so that several tiles' passes overlap).
 *   SPHX_ERR_NOT_READY between a halo exchange and the tile's re-grid.  sphx_tile_upload_state is sphx_tile_upload that also installs the
 *   two warm-start arrays (NULL: zeros). */
#define SPHX_MULTI_STATE_SECTIONS 8
enum {
    SPHX_MULTI_STATE_SEC_POSITIONS = 0, SPHX_MULTI_STATE_SEC_VELOCITIES = 1, SPHX_MULTI_STATE_SEC_PARTICLE_ID = 2, SPHX_MULTI_STATE_SEC_DENSITY = 3,
    SPHX_MULTI_STATE_SEC_ALPHA = 4, SPHX_MULTI_STATE_SEC_KAPPA = 5, SPHX_MULTI_STATE_SEC_STIFFNESS = 6, SPHX_MULTI_STATE_SEC_BOUNDARY = 7
};
enum { SPHX_TILE_STATE_ZERO_KAPPA = 1u, SPHX_TILE_STATE_ZERO_STIFFNESS = 2u };
typedef struct sphx_tile_state_out { /* device pointers, n_owned entries each */
    const float* pos;                /* xy */
    const float* vel;                /* xy */
    const uint32_t* id;              /* bit 31 cleared */
    const float *density, *alpha, *kappa, *stiffness;
} sphx_tile_state_out;
int sphx_tile_state_pack(sphx_ctx* tile_ctx, uint32_t flags, sphx_tile_state_out* out, uint64_t* out_digests /* [7], may be NULL */,
                         uint32_t* out_n_owned /* may be NULL */);
int sphx_tile_state_fetch(sphx_ctx* tile_ctx, uint64_t* out_digests /* [7], may be NULL */, uint32_t* out_n_owned /* may be NULL */);
int sphx_tile_upload_state(sphx_ctx* ctx, const float* pos_xy, const float* vel_xy, const uint32_t* ids, const float* kappa, const float* stiffness, uint32_t n);
int sphx_get_tiling_invariant(const sphx_ctx* ctx); /* 1 in tiling-invariant mode, else 0 */
int sphx_multi_state_size(sphx_multi* m, uint64_t* out_bytes);
int sphx_multi_state_save(sphx_multi* m, void* buf /* host */, uint64_t capacity, uint32_t flags /* 0 */, uint64_t* out_bytes /* may be NULL */);
int sphx_multi_state_load(sphx_multi* m, const void* const* parts /* host */, const uint64_t* bytes, uint32_t n_parts, uint32_t flags /* 0 */);
int sphx_multi_state_digest(sphx_multi* m, uint64_t* out /* [SPHX_MULTI_STATE_SECTIONS]: the whole run; collective in rank mode */);
int sphx_multi_state_save_file(sphx_multi* m, const char* path); /* rank mode: path + ".rRRRofWWW" */
int sphx_multi_state_load_file(sphx_multi* m, const char* path); /* the one file, or the complete set of part files */

/* ---- emitting and draining fluid in a tiled run (csrc/sphx_multi_edit.inc, csrc/sphx_multi_edit.hpp, csrc/sphx_tiles.cpp) ---------------------
 * sphx_append / sphx_remove for a sphx_multi: an inflow, an outflow or a keep-box without the round trip sphx_multi_download, edit on the
 * host, sphx_multi_upload (36 bytes per particle over PCIe, a fresh decomposition on every rank, renumbered ids, warm-start sums and
 * iteration counts lost).  Both calls are COLLECTIVE in rank mode: every rank calls with the same arguments.  The contract:
 *   Predicate and arguments (sphx_multi_remove): exactly sphx_remove's — the same fp32 comparisons, a NaN coordinate is in no rectangle,
 *     SPHX_REMOVE_OUTSIDE makes the rectangles a keep-box, at most SPHX_REMOVE_MAX_RECTS rectangles; a NaN bound, too many rectangles,
 *     rects NULL with n_rects > 0 or unknown flag bits: SPHX_ERR_INVALID_ARGUMENT.  The predicate looks at positions only: an owner and
 *     every tile that holds a ghost of its particle see the same bits, so no tile has to tell another which particles went.
 *   Remove: every tile retires those of the records it OWNS (bit 31 of its id word) that the predicate removes — position x becomes NaN,
 *     the form in which the halo exchange already drops a record — and counts them.  A record whose x is NaN already was retired before: it
 *     is not counted (and no particle with a NaN x is ever counted, whatever SPHX_REMOVE_OUTSIDE says).  The counts are summed over all
 *     tiles (rank mode: one all-reduce); *out_removed (may be NULL) is that sum, the same on every rank, and whether anything was removed
 *     is decided from it alone.
 *       sum == 0: the multi is untouched — no exchange, no re-grid, sphx_multi_info().exchanges unchanged; lists, recorders and a queued
 *         run-ahead pass stay valid.
 *       sum > 0: every tile runs one halo exchange and one re-grid (exchanges grows by exactly 1).  The survivors keep position, velocity,
 *         id, kappa and stiffness bit for bit; density and alpha are recomputed for the whole local set.
 *   Append: in rank mode every rank is handed the same n_new records, as sphx_multi_upload is.  A non-finite position is
 *     SPHX_ERR_INVALID_ARGUMENT before anything changes (a NaN x is the retired mark).  Record k gets the id first_id + k, where first_id =
 *     *out_first_id (may be NULL) = the multi's id counter: n after sphx_multi_upload with ids == NULL, 1 + the greatest id after one with
 *     ids and after sphx_multi_state_load (1 + the greatest id in the checkpoint); it grows by n_new.  An id at or above 2^31 is
 *     SPHX_ERR_CAPACITY with nothing changed.  The checkpoint format has no field for the counter: ids are unique among the LIVE particles
 *     always, and never reused within a run that does not load a checkpoint — after a load, the id of a particle removed before the save may
 *     be handed out again.  Each record goes to the tile whose rectangle holds its cell under the CURRENT layout (after rebalances), the
 *     rule of the upload's decomposition; the owner stores it behind its local set with the owner bit, the velocity (vel_xy NULL: zero) and
 *     kappa = stiffness = +0.0.  A tile whose capacity does not hold its local set, the routed records and the room of one halo exchange
 *     grows its arrays by half (at least to what is needed), the present records and their warm-start sums copied on the device.  Then every
 *     tile runs one halo exchange and one re-grid: the ghosts of the new particles appear on the neighbours in that same exchange.
 *     n_new == 0 leaves the multi untouched and still reports first_id.  The caller's arrays are borrowed for the duration of the call.
 *   Both calls keep the iteration counts (warm starts), the step count, the layout, the halo width in use and the recorders
 *     (sphx_multi_stats_record).  sphx_multi_num_owned and the global count are exact after the call (no particle migrates in an edit's
 *     exchange: positions have not moved since the step's own).  sphx_multi_download, _render, _fluid_stats, _state_save and _state_digest
 *     work at once on the new set.  No flag is raised: there is no SPHX_FLAG_WARMUP, the re-grid of the exchange is the warm-up block.
 *   Equivalence: the state after an edit is the state that sphx_multi_state_save, dropping the removed particles from the sections (or
 *     adding the new records with kappa = stiffness = 0), sphx_multi_state_load leaves in a multi with the same tiling.  In tiling-invariant
 *     mode with fixed iteration counts every later step is bit-identical to that run's, and the run does not depend on the tiling.  In
 *     default mode the edit holds the surviving particles bit for bit and the run continues as a valid run of that state (the wording of
 *     the checkpoint's contract).
 *   Refusals: SPHX_ERR_NOT_READY between sphx_multi_step_begin and _finish, before the first sphx_multi_upload or sphx_multi_state_load,
 *     after a load that did not complete and after a failed collective step.  A refused call leaves the multi untouched.
 *   Limit: the halo buffers keep the capacity the upload estimated from its scene (1.5 x the estimate + 1 024 records, or
 *     sphx_multi_options.cap_records).  An emitter that fills a send band beyond it raises the halo-capacity condition in the step, as
 *     a compression wave would; the buffers are not re-sized after an edit — cap_records is the knob.
 * Cost: a removal reads 12 bytes per local record (id + position) and writes 4 per removed one; one 4-byte count per tile comes back.
 * Nothing removed: that is all.  Otherwise one halo exchange + re-grid, what a step pays once.
 * INTERNAL seam (the tile loop, and drivers in the style of tests/tiles_reference.py).  sphx_tile_remove_mark enqueues the pass on the
 * tile's stream and waits for nothing; sphx_tile_remove_fetch brings the one word back (the pair lets tiles on different devices
 * overlap).  sphx_tile_append stores owned records (ids below 2^31, finite positions) behind the local set, growing the arrays when they do
 * not fit; sphx_tile_grow makes room for `capacity` records in all (the halo's room included) ahead of it.  After a fetch that returned
 * > 0 and after an append the tile is between a halo exchange and its re-grid: sphx_tile_pack_n ... sphx_sub_regrid come next. */
int sphx_multi_append(sphx_multi* m, const float* pos_xy, const float* vel_xy /* NULL = 0 */, uint32_t n_new, uint32_t* out_first_id /* may be NULL */);
int sphx_multi_remove(sphx_multi* m, const sphx_rect* rects, uint32_t n_rects, uint32_t flags, uint64_t* out_removed /* may be NULL */);
int sphx_tile_remove_mark(sphx_ctx* tile_ctx, const sphx_rect* rects, uint32_t n_rects, uint32_t flags);
int sphx_tile_remove_fetch(sphx_ctx* tile_ctx, uint32_t* out_removed_owned);
int sphx_tile_append(sphx_ctx* tile_ctx, const float* pos_xy, const float* vel_xy /* NULL = 0 */, const uint32_t* ids, uint32_t n_new);
int sphx_tile_grow(sphx_ctx* tile_ctx, uint32_t capacity);

/* ---- neighbour queries of a tiled run (csrc/sphx_tiles.cpp; device passes csrc/sphx_query.inc, the fold csrc/sphx_query_merge.hpp;
 * DESIGN.md section 4s) ------------------------------------------------------------------------------------------------------------
 * sphx_query_radius / sphx_select for a sphx_multi, without sphx_multi_download and a second context.
 * sphx_multi_query_radius:
 * Who answers: the tile whose owned cell rectangle contains cell_of(q), as in "sampling the fields of a tiled run": exactly one tile
 *   per point.  A NaN coordinate goes to cell 0 and fails every distance test, as in the single call.
 * What it computes: the contract of sphx_query_radius, word for word, over THAT TILE'S OWN ARRAYS — candidates, acceptance, entry
 *   order, nearest and its tie rule, the box rule, the radius rule and the capacity rule (nothing at or behind cap_entries is ever
 *   written; offsets and count describe the FULL result).  Ghosts are candidates like any other particle.  With SPHX_QUERY_BOUNDARY the
 *   set is the tile's clipped boundary.  Consequences: (a) in every mode the result is bit-identical to the restatement of that
 *   contract (tests/query_reference.py) over the answering tile's own downloads, ids translated as below; (b) in tiling-invariant mode
 *   offsets, id, dist_sq, nearest_id, nearest_dist_sq and count are byte for byte those of sphx_query_radius on a single context in the
 *   same mode (slot is tile-local by definition); (c) for radius <= 0.9 * smoothing_length the result is every particle of the whole
 *   run within the radius, whatever the tiling (a margin of 0.1 cell, far more than the rounding of the cell function: about 1e-3 cell
 *   at the reference's grid origin).
 * Ids: a fluid entry carries the particle id as sphx_multi_download reports it (owner bit cleared; the candidate may be a ghost).  A
 *   boundary entry carries the index of the particle in the array given to sphx_multi_set_boundary: every tile keeps the map from its
 *   clipped set to the caller's order, renewed whenever the boundary is clipped again (a re-partition), and the host translates.
 *   slot is the index in the ANSWERING tile's own download (sphx_download / sphx_download_boundary on sphx_multi_tile_ctx).
 * The ghost band: unlike sampling, a query reads only positions and ids of ring-1 ghosts.  Positions of ghosts are exact after every
 *   exchange, and at every point where the call is allowed no advection is pending (a finished step's own exchange has applied it).  So
 *   no halo exchange is ever triggered, the call only reads (the sweep direction is put back), sphx_multi_info().exchanges never moves
 *   and the call is NOT COLLECTIVE: a rank may call alone, with points of its own.
 * When allowed: after sphx_multi_upload, after every finished step and after sphx_multi_append / _remove / _state_load — each of them
 *   ends with the re-grid of every tile, which is all the tile's state test asks for (the cell grids belong to the positions, no
 *   advection pending, no step open): they hold without a refresh.  SPHX_ERR_NOT_READY where sphx_multi_sample_points returns it.
 * A tile without any particle answers with empty lists over the fluid, and over its static grid with SPHX_QUERY_BOUNDARY.
 * SPHX_ERR_INVALID_ARGUMENT (sphx_multi_last_error names the argument): m, out or out->count NULL, xy NULL with m > 0, m >= 2^31, a bad
 *   radius, any flag bit but SPHX_QUERY_BOUNDARY, more than 64 tiles, rank mode without out->tile.  A refused call touches no tile.
 *   m == 0 succeeds with *count = 0 (and offsets[0] = 0).
 * Determinism: no atomic decides a position; two calls return the same bytes.
 * In-process (sphx_multi_create): every point is answered; out->tile is optional.  Rank mode (sphx_multi_create_rank): the call returns
 *   this rank's part — offsets over the rank's own entries, a point the rank does not answer has an empty range, tile = -1, nearest_*
 *   SPHX_QUERY_NONE and +inf; count is the rank's total.  sphx_query_merge(m, parts, parts_cap, n_parts, cap_entries, out) folds such
 *   parts into one result in the caller's order: pure host code; per point the part with tile >= 0, the lowest tile if several have
 *   one, an empty range and -1 if none.  A part holds min(its count, parts_cap[p]) entries; if the result needs an entry that a part
 *   truncated the call returns SPHX_ERR_CAPACITY.  Every part carries offsets, tile and the arrays out asks for; n_parts == 0 gives the
 *   all-absent answer; nothing at or behind cap_entries is written.
 * sphx_multi_select: sphx_remove's predicate, bit for bit, evaluated by every tile on the particles it OWNS (a ghost never answers),
 *   in the order of sphx_multi_download — tiles in rank order, each in ascending local index; tile and slot say where each particle
 *   lives, id is the id with the owner bit cleared.  count is 64-bit; the capacity rule is that of the query.  Allowed wherever
 *   sphx_multi_download is (SPHX_ERR_NOT_READY inside an open step and before the first upload); it only reads.  Rank mode: this rank's
 *   part; the whole answer is the parts concatenated in rank order, as for sphx_multi_particle_fields.  Argument errors: sphx_select's
 *   (without a device-pointer flag), more than 64 tiles.
 * Device work per tile: all m points go up (8 bytes each); a stable selection (count per workgroup, scan, write) lists the points the
 *   tile owns in ascending index; the counting and the emitting walk of sphx_query_radius run over that list with every lane live, so
 *   the K tiles together walk m points; per answered point 24 bytes and per kept entry 12 bytes come back.  Figures: DESIGN.md 4s.
 * One tile (INTERNAL, accepted only on a tile context — sphx_query_radius and sphx_select keep refusing one):
 *   sphx_tile_query_radius enqueues upload, selection and the counting walk.  sphx_tile_query_fetch is called twice: with part->point
 *   and part->offset NULL it reads the two totals (the one synchronisation), enqueues the emitting walk for kept = min(total,
 *   cap_entries) entries and reports n_points, total and kept; with arrays of those sizes it copies the records (point: ascending point
 *   indices; offset: the tile-local first entry of each) and the kept entries, and ends the query.  sphx_tile_select enqueues the flag
 *   and scan passes; sphx_tile_select_fetch reports the total and, given cap > 0 and an array, emits and copies min(total, cap) pairs
 *   (it may be called again until the next enqueue). */
typedef struct sphx_multi_query_out {      /* host arrays */
    uint64_t* offsets;          /* [m+1] CSR over the caller's points, or NULL */
    uint32_t* id;               /* [cap_entries] particle id as sphx_multi_download reports it (owner bit cleared); with
                                   SPHX_QUERY_BOUNDARY the index of the particle in the array given to sphx_multi_set_boundary; or NULL */
    float*    dist_sq;          /* [cap_entries] or NULL */
    uint32_t* slot;             /* [cap_entries] index in the ANSWERING tile's own download (sphx_multi_tile_ctx; boundary: in its
                                   sphx_download_boundary), or NULL */
    uint32_t* nearest_id;       /* [m]  SPHX_QUERY_NONE if none, or NULL */
    uint32_t* nearest_slot;     /* [m]  likewise, or NULL */
    float*    nearest_dist_sq;  /* [m]  0x7F800000 if none, or NULL */
    int32_t*  tile;             /* [m]  global rank of the answering tile, -1: none of the local tiles; required in rank mode */
    uint64_t* count;            /* [1]  total entries; required */
} sphx_multi_query_out;         /* 72 bytes */
int sphx_multi_query_radius(sphx_multi* m, const float* xy /* host */, uint32_t n, float radius, uint64_t cap_entries,
                            uint32_t flags /* SPHX_QUERY_BOUNDARY or 0 */, const sphx_multi_query_out* out);
int sphx_query_merge(uint32_t m, const sphx_multi_query_out* parts, const uint64_t* parts_cap, uint32_t n_parts, uint64_t cap_entries,
                     const sphx_multi_query_out* out);   /* pure host code */
typedef struct sphx_multi_select_out {
    uint32_t* id;     /* [cap] or NULL */
    int32_t*  tile;   /* [cap] global rank of the owning tile, or NULL */
    uint32_t* slot;   /* [cap] index in that tile's own download, or NULL */
    uint64_t* count;  /* [1] number selected by the local tiles; required */
} sphx_multi_select_out;        /* 32 bytes */
int sphx_multi_select(sphx_multi* m, const sphx_rect* rects, uint32_t n_rects, uint32_t flags /* SPHX_SELECT_OUTSIDE or 0 */, uint64_t cap,
                      const sphx_multi_select_out* out);
typedef struct sphx_tile_query_part {      /* host arrays */
    uint32_t  n_points;         /* out: points this tile answers */
    uint32_t  reserved;
    uint64_t  total;            /* out: their entries */
    uint64_t  kept;             /* out: min(total, cap_entries) */
    uint32_t* point;            /* [n_points] ascending point indices */
    uint64_t* offset;           /* [n_points] first entry of each, tile-local */
    uint32_t* nearest_slot;     /* [n_points] each, or NULL */
    uint32_t* nearest_id;
    float*    nearest_dist_sq;
    uint32_t* slot;             /* [kept] each, or NULL */
    uint32_t* id;
    float*    dist_sq;
} sphx_tile_query_part;         /* 88 bytes */
int sphx_tile_query_radius(sphx_ctx* tile_ctx, const float* xy /* host, [2m] */, uint32_t m, float radius, uint32_t flags, uint32_t want_nearest);
int sphx_tile_query_fetch(sphx_ctx* tile_ctx, uint64_t cap_entries, sphx_tile_query_part* part);
int sphx_tile_select(sphx_ctx* tile_ctx, const sphx_rect* rects, uint32_t n_rects, uint32_t flags);
int sphx_tile_select_fetch(sphx_ctx* tile_ctx, uint32_t cap, uint32_t* slot /* host, [cap] */, uint32_t* id, uint32_t* out_total);

/* ---- gauges and probes of a tiled run (csrc/sphx_gauge.inc, csrc/sphx_gauge_window.hpp, csrc/sphx_gauge_merge.hpp) -----------------------
 * sphx_gauge_levels and the sphx_probe_* recorder for a sphx_multi.  Every sample of a ray and every probe point is answered by the tile
 * that owns its cell, over that tile's own arrays — the bits sphx_multi_sample_points returns at that point.  The values stay on the
 * devices: each tile reduces the samples it owns on a gauge to one 32-byte sphx_gauge_part, and a pure host fold makes the record.
 * Two facts carry this (stated and proved in sphx_gauge_window.hpp, held by tests/test_gauge_multi_host.py before any kernel runs):
 *   1. the owned samples of one tile on one gauge are one contiguous index interval [lo, lo + count), found by four bisections on the
 *      host, for steps of either sign, zero steps and coordinates that overflow;
 *   2. the intervals of the tiles partition [0, n); if the tile that owns sample `last` does not own last + 1, then last + 1 is the
 *      first owned sample of the tile that does.  So a part that carries the value at its own first sample is enough.
 * sphx_gauge_part (one per tile and gauge): lo, count = the owned interval in global sample indices, count being the number of samples
 *   the DEVICE's ownership test (the tile rectangle over cell_of) accepted; first, last, inside over the owned samples, as global
 *   indices (SPHX_GAUGE_NONE / 0 if none); f_lo = the value at sample lo; f_last = the value at the part's own last; f_next = the value at
 *   its own last + 1 if the part owns that sample.  A member without a meaning holds the word 0x7FC00000.
 * The fold: the parts with count > 0, ordered by lo, must tile [0, n) exactly — a gap, an overlap or a count that disagrees with the
 *   host's interval is an error (SPHX_ERR_HIP from the multi, SPHX_ERR_INVALID_ARGUMENT from sphx_gauge_merge) and no record is
 *   returned.  Then first = the minimum, last = the maximum, inside = the sum, f_last from the part that holds last, f_next from that part
 *   or from the f_lo of the part whose lo == last + 1, and the record is formed by the one function that forms it everywhere
 *   (sphx_gauge_rule.hpp): bit for bit sphx_gauge_reduce over the concatenated values.  Consequences: the records equal the gauge rule
 *   over sphx_multi_sample_points' values; in tiling-invariant mode they equal sphx_gauge_levels on a single context byte for byte.
 * sphx_multi_gauge_levels: arguments, limits and messages of sphx_gauge_levels (flags must be 0: there is no device-pointer path across
 *   several devices).  State rules and the ghost band: those of sphx_multi_sample_points — if the band is spent, the halo exchange the
 *   next step owes happens now, and the run is unchanged; the call is collective in rank mode for that reason.  All local tiles
 *   enqueue, then the parts (and the compact values, if asked for) are fetched and folded.  values: host, [sum n] — tile t's values of
 *   gauge g arrive at offset(g) + lo; in rank mode the samples other ranks own are left as they were.  out_parts: host, [local
 *   tiles][n_gauges], or NULL.  In rank mode out_parts is required, out may be NULL and is not written: the caller moves the parts and
 *   folds them with sphx_gauge_merge(gauges, n_gauges, iso, parts, n_parts, out) — parts is [n_parts][n_gauges] — pure host code.
 * The recorder: sphx_multi_probe_record(points, m_points, gauges, n_gauges, ..., max_frames, every) — arguments, limits, `dropped`,
 *   max_frames == 0 and "a new record discards the old" as sphx_probe_record; the 64 MiB cap is per tile.  Every every-th finished
 *   multi step (also each step inside sphx_multi_simulation_steps) takes a frame on every tile, behind the tile's own kernels: the
 *   ghost band is made final the way a query does (the exchange the next step owes, if the band is spent — the next step then makes
 *   none), then the tile enqueues its passes.  Nothing else is synchronised; the parts are folded at the read.  The cuts move: a tile's
 *   interval table is rebuilt on the host and re-sent as kernel arguments whenever the tile's owned rectangle differs from the one
 *   the table was built for, checked at every frame.  It may be called before the first upload.  The recording belongs to the
 *   MULTI: it survives migration, re-partitioning, sphx_multi_append / _remove, uploads and state loads.
 *   sphx_multi_probe_read(first, n, points_out, point_tile, gauges_out, info): points_out [n][m_points] sphx_probe_rec folded by the
 *   tiles' "answered" mark, lowest tile first (reserved words zero; nobody answered: zeros), point_tile [n][m_points] the tile that
 *   answered or -1, gauges_out [n][n_gauges] folded records.  Rank mode: points_out / point_tile are this rank's part (fold by
 *   point_tile >= 0), gauges_out must be NULL — the rank's parts come from sphx_tile_probe_read on sphx_multi_tile_ctx.
 * No side effects: a run with a recording and one-shot calls is bit-identical to the run without, exchanges and rebalances included.
 * One tile (INTERNAL, accepted only on a tile context — sphx_gauge_levels and sphx_probe_* keep refusing one): sphx_tile_gauge_levels
 *   enqueues the table, the sample pass over the owned samples and the reduce pass; sphx_tile_gauge_fetch copies the parts (and the
 *   compact values: the owned samples gauge after gauge) and checks the device's counts against the host's intervals.
 *   sphx_tile_probe_record / _due / _frame / _read are the seam of the recorder; a stored point slot carries the "answered" mark in
 *   reserved[0]. */
typedef struct sphx_gauge_part {      /* 32 bytes */
    uint32_t lo, count;               /* the owned interval [lo, lo + count) */
    uint32_t first, last, inside;     /* over the owned samples, global indices */
    float f_lo, f_last, f_next;       /* values at lo, at last, at last + 1 (if owned) */
} sphx_gauge_part;
int sphx_multi_gauge_levels(sphx_multi* m, const sphx_gauge* gauges /* host */, uint32_t n_gauges, int kernel_kind, int field, float iso,
                            uint32_t flags /* 0 */, sphx_gauge_rec* out /* [n_gauges] */, float* values /* host [sum n] or NULL */,
                            sphx_gauge_part* out_parts /* [local tiles][n_gauges] or NULL */);
int sphx_gauge_merge(const sphx_gauge* gauges, uint32_t n_gauges, float iso, const sphx_gauge_part* parts /* [n_parts][n_gauges] */,
                     uint32_t n_parts, sphx_gauge_rec* out /* [n_gauges] */);   /* pure host code */
int sphx_multi_probe_record(sphx_multi* m, const float* points_xy /* host */, uint32_t m_points, const sphx_gauge* gauges /* host */,
                            uint32_t n_gauges, int kernel_kind, int field, float iso, uint32_t max_frames, uint32_t every);
int sphx_multi_probe_get_status(const sphx_multi* m, sphx_probe_status* out);
int sphx_multi_probe_read(sphx_multi* m, uint32_t first_frame, uint32_t n_frames, sphx_probe_rec* points_out /* [n_frames][m_points] or NULL */,
                          int32_t* point_tile /* [n_frames][m_points] or NULL */, sphx_gauge_rec* gauges_out /* [n_frames][n_gauges] or NULL */,
                          sphx_stats_frame* info /* [n_frames] or NULL */);
int sphx_tile_gauge_levels(sphx_ctx* tile_ctx, const sphx_gauge* gauges /* host */, uint32_t n_gauges, int kernel_kind, int field, float iso);
int sphx_tile_gauge_fetch(sphx_ctx* tile_ctx, sphx_gauge_part* parts /* host, [n_gauges] */, float* values /* host, compact, or NULL */,
                          uint32_t* out_lo_count /* host, [2 n_gauges]: the host's intervals, or NULL */);
int sphx_tile_probe_record(sphx_ctx* tile_ctx, const float* points_xy, uint32_t m_points, const sphx_gauge* gauges, uint32_t n_gauges,
                           int kernel_kind, int field, float iso, uint32_t max_frames, uint32_t every);
int sphx_tile_probe_due(const sphx_ctx* tile_ctx);  /* 1: the next sphx_tile_probe_frame stores a frame */
int sphx_tile_probe_frame(sphx_ctx* tile_ctx, float dt, uint32_t n_global); /* one finished step: a frame if the recording is due */
int sphx_tile_probe_read(sphx_ctx* tile_ctx, uint32_t first_frame, uint32_t n_frames, sphx_probe_rec* points_out /* marks kept */,
                         sphx_gauge_part* parts_out /* [n_frames][n_gauges] */, sphx_stats_frame* info);

/* ---- single-node scalar reductions through POSIX shared memory ---------------------------------------------------------------
 * The three per-step scalars of the tile driver (vmax, two residual sums) already sit in host memory (pinned mailbox) on every
 * rank; for one process per GPU on ONE node a shared-memory all-reduce costs ~1 us instead of a device round trip through
 * RCCL.  RCCL is used where the path really exchanges data (the halo records).  name: unique per job (e.g. MASTER_PORT). */
typedef struct sphx_shm sphx_shm;
/* Collective: every rank of the run calls it (in any order); it returns once all `world` ranks have joined the SAME segment — rank 0
 * replaces whatever an earlier run left under the name, a rank that attached to such a leftover notices (nobody answers its join
 * token) and attaches again.  NULL on failure or when a rank does not show up within min(SPHX_SHM_TIMEOUT_S, 120) seconds. */
sphx_shm* sphx_shm_open(const char* name, int rank, int world);
/* op: 0 = sum, 1 = max; n <= 8 doubles; every rank gets the same bits (ranks are combined in rank order).  Returns
 * SPHX_ERR_NOT_READY — on every waiting rank, at once — when a rank has called sphx_shm_abort / sphx_shm_close instead of arriving, or
 * after SPHX_SHM_TIMEOUT_S seconds (default 300) without it. */
int sphx_shm_allreduce(sphx_shm* h, const double* in, int n, int op, double* out);
/* every rank's n <= 8 doubles to every rank: out[r * n + k] = rank r's in[k] (world * n doubles).  Same failure behaviour.  The tile
 * driver publishes the record counts of its halo messages this way, so that ncclSend / ncclRecv move what was packed, not the
 * buffers' capacity. */
int sphx_shm_allgather(sphx_shm* h, const double* in, int n, double* out);
void sphx_shm_abort(sphx_shm* h); /* this rank has failed: release the ranks that wait for it */
void sphx_shm_close(sphx_shm* h);

/* NOT the reference's behaviour — a comparison mode for multi-GPU runs.  Two things in a DFSPH run depend on how the domain is cut into
 * tiles: the order of the particles inside a cell (the reference's par_sort_unstable_by_key leaves it open, neighborhood_search.rs:118;
 * this build keeps them in the order of their previous index, which a tile that appends what it receives cannot reproduce) and the
 * warm-start values, which the reference leaves bound to their slot when the particles are re-sorted (dfsph.rs:512) — a slot means
 * nothing across tiles, so tiles let them travel with the particle.  With this switch a context orders the particles of a cell by their
 * persistent id (sphx_download's particle_id) and moves the warm-start values with them: a single context, any sphx_multi tiling and
 * the oracle in the same mode then compute the same run (tests/test_gpu_tiles_full.py, tests/test_gpu_multi.py at 64 M / 128 M).  Off by
 * default; tile contexts take the switch for the cell order (their warm-start values always travel).  Two exceptions: particles with
 * EQUAL ids (caller-supplied through sphx_multi_upload) keep their previous order among themselves, and a cell with more than 4 096
 * particles (a collapse to a point; SPHX_FLAG_DENSE_CELL) keeps arrival order — for those the run may depend on the tiling. */
int sphx_set_tiling_invariant(sphx_ctx* ctx, int on);

/* ---- measurement ---------------------------------------------------------------------------------------------- */
int sphx_synchronize(sphx_ctx* ctx);
/* the latest neighbour build of this context: particles it ran over, list entries in total, entries outside the workgroup windows */
int sphx_build_stats(const sphx_ctx* ctx, uint32_t* out_particles, uint64_t* out_entries, uint64_t* out_remote);
/* Run this context on a HIP stream owned by the caller (hipStream_t; NULL = back to a private stream).  The tile driver passes
 * the stream RCCL orders its sends/receives against, so packing, exchange and unpacking need no host synchronisation. */
int sphx_set_stream(sphx_ctx* ctx, void* hip_stream);
/* When enabled every kernel launch is bracketed by hipEvents on the context's stream; totals are kept per kernel name. */
int sphx_profile_enable(sphx_ctx* ctx, int on);
int sphx_profile_reset(sphx_ctx* ctx);
int sphx_profile_filter(sphx_ctx* ctx, const char* label, uint32_t every); /* time only every `every`-th launch with this label (NULL = all
                                                                              launches): light enough for a timed region */
/* Fills up to *inout_n records; names are NUL-terminated, <= 47 chars. */
typedef struct sphx_kernel_time {
    char name[48];
    uint64_t launches;
    double total_ms;
    double algorithmic_bytes; /* sum over launches of the algorithmic byte count of DESIGN.md */
} sphx_kernel_time;
int sphx_profile_get(sphx_ctx* ctx, sphx_kernel_time* out, uint32_t* inout_n);
/* what the hipEvent bracket itself adds to a measured launch: mean elapsed time between the two events of an EMPTY bracket */
int sphx_profile_event_overhead(sphx_ctx* ctx, double* out_ms);

/* ======================================================================================================================
 * Host-side mirror of the reference's caller-side types (scene helpers, TimeManager, Solver object).  These exist so the
 * C++ harness / Python drivers can play the role of the Rust application; a Rust host would keep using its own types.
 * ====================================================================================================================== */
typedef struct sphx_world sphx_world;   /* FluidParticleWorld (fluidparticleworld.rs:92-102) host arrays + properties */
typedef struct sphx_timer sphx_timer;   /* TimeManager (timemanager.rs:72-92), simulation-step part only */
typedef struct sphx_solver sphx_solver; /* Box<dyn Solver> (main.rs:50): HIP-backed DFSPHSolver */

sphx_world* sphx_world_create(float smoothing_factor, float particle_density, float fluid_density); /* fluidparticleworld.rs:104 */
void sphx_world_destroy(sphx_world* w);
void sphx_world_properties(const sphx_world* w, float* out4); /* {smoothing_length, particle_mass, particle_radius, fluid_density} */
void sphx_world_remove_all_fluid_particles(sphx_world* w);    /* fluidparticleworld.rs:129-132 */
void sphx_world_remove_all_boundary_particles(sphx_world* w); /* fluidparticleworld.rs:134-137 */
void sphx_world_add_fluid_rect(sphx_world* w, float x, float y, float width, float height, float jitter_amount); /* :140-166 */
void sphx_world_add_boundary_thick_line(sphx_world* w, float sx, float sy, float ex, float ey, uint32_t thickness); /* :168-179 */
void sphx_world_add_boundary_line(sphx_world* w, float sx, float sy, float ex, float ey); /* :181-195 */
/* main.rs:177-196 `reset_fluid` with every coordinate multiplied by `scale` (scale 1 = the reference scene, ~4050 particles) */
void sphx_world_reset_fluid(sphx_world* w, float scale);
uint32_t sphx_world_num_dynamic_particles(const sphx_world* w);  /* fluidparticleworld.rs:37 */
uint32_t sphx_world_num_boundary_particles(const sphx_world* w); /* fluidparticleworld.rs:41 */
float* sphx_world_positions(sphx_world* w);   /* interleaved xy, length 2*num_dynamic */
float* sphx_world_velocities(sphx_world* w);
float* sphx_world_densities(sphx_world* w);
float* sphx_world_boundary(sphx_world* w);
uint32_t* sphx_world_particle_ids(sphx_world* w); /* valid after a solver step with sync enabled */
void sphx_world_set_particles(sphx_world* w, const float* pos_xy, const float* vel_xy, uint32_t n);
void sphx_world_set_boundary(sphx_world* w, const float* xy, uint32_t n);
void sphx_world_set_gravity(sphx_world* w, float gx, float gy);

uint64_t sphx_duration_from_secs_f32(float secs); /* std::time::Duration::from_secs_f32 -> nanoseconds (round-to-nearest-even) */
float sphx_duration_as_secs_f32(uint64_t nanos);  /* Duration::as_secs_f32 */
sphx_timer* sphx_timer_create_adaptive(uint64_t timestep_max_ns, uint64_t timestep_min_ns, float cfl_factor); /* timemanager.rs:44-58,105-129 */
sphx_timer* sphx_timer_create_fixed(uint64_t timestep_ns);                                                     /* timemanager.rs:40 */
void sphx_timer_destroy(sphx_timer* t);
void sphx_timer_restart(sphx_timer* t);                                                     /* timemanager.rs:131-133 */
uint64_t sphx_timer_simulation_step_ns(const sphx_timer* t);                                /* timemanager.rs:136-138 */
uint64_t sphx_timer_update_simulation_step(sphx_timer* t, float particle_diameter, float max_velocity); /* timemanager.rs:252-279 */
uint64_t sphx_timer_total_simulated_ns(const sphx_timer* t);
uint32_t sphx_timer_num_steps(const sphx_timer* t);
int sphx_timer_law_of(const sphx_timer* t, float particle_diameter, sphx_timer_law* out); /* fills sphx_timer_law from the mirror */
void sphx_timer_set_target_frame(sphx_timer* t, uint64_t target_ns); /* AdaptiveTimeStepTarget::TargetFrameLength, timemanager.rs:24-36; 0 = None */
void sphx_timer_on_step_started(sphx_timer* t);                      /* the clock part of simulation_frame_loop, timemanager.rs:244-247 */
/* Everything the TimeManager mirror holds (timemanager.rs:72-92, simulation-step part), as one POD: a timer given the state of another
 * continues exactly as that one would.  sphx_timer_set_state: SPHX_ERR_INVALID_ARGUMENT for NULL, fixed > 1, reserved != 0 or a NaN factor. */
typedef struct sphx_timer_state {
    uint32_t fixed;                     /* SimulationStepConfig::Fixed (1) or ::Adaptive (0) */
    float cfl_factor;
    uint64_t timestep_max_ns, timestep_min_ns;
    uint64_t simulation_step_ns;        /* TimeManager::simulation_step() */
    uint64_t timestep_target_frame_ns;  /* AdaptiveTimeStepTarget::TargetFrameLength; 0 = None */
    uint64_t total_simulated_ns;
    uint32_t num_simulation_steps;
    uint32_t reserved;                  /* 0 */
} sphx_timer_state;                     /* 56 bytes */
int sphx_timer_get_state(const sphx_timer* t, sphx_timer_state* out);
int sphx_timer_set_state(sphx_timer* t, const sphx_timer_state* state);

/* DFSPHSolver::new(XSPHViscosityModel::new(h), h) boxed as dyn Solver (main.rs:93-101).  `params` may be NULL (defaults from the world). */
int sphx_solver_create_dfsph(const sphx_world* w, const sphx_params* params, sphx_solver** out);
int sphx_solver_create_wcsph(const sphx_world* w, const sphx_params* params, sphx_solver** out); /* WCSPHSolver::new, wscsph.rs:29-42 */
/* the same Box<dyn Solver> over several GPUs (one tile per entry of devices[]; sphx_multi inside): the caller's loop does not change */
int sphx_solver_create_dfsph_multi(const sphx_world* w, const sphx_params* params, const int* devices, int n_devices,
                                   const sphx_multi_options* options, sphx_solver** out);
void sphx_solver_destroy(sphx_solver* s);
void sphx_solver_clear_cached_data(sphx_solver* s); /* Solver::clear_cached_data */
/* Solver::simulation_step(&mut world, &mut time_manager) (dfsph.rs:414).  sync_world != 0 copies positions/velocities/
 * densities back into the host world before returning (what main.rs:242-258 draws from); 0 keeps them device-resident. */
int sphx_solver_simulation_step(sphx_solver* s, sphx_world* w, sphx_timer* t, int sync_world, sphx_step_stats* out_stats);
/* `k` consecutive simulation_step calls — the frame loop of main.rs:348-350 (PerformStepAndCallAgain -> single_sim_step, :279) on
 * this side of the boundary, for hosts whose per-call cost matters (a Python driver: ~8 us a step at 1 M particles).  Nothing is
 * skipped or batched on the device: it IS the loop `for _ in 0..k { solver.simulation_step(world, timer) }`.  out_stats: k entries
 * or NULL; *out_done (may be NULL) = steps finished; stops at the first failing step and returns its code. */
int sphx_solver_simulation_steps(sphx_solver* s, sphx_world* w, sphx_timer* t, int sync_world, uint32_t k, sphx_step_stats* out_stats,
                                 uint32_t* out_done);
int sphx_solver_sync_world(sphx_solver* s, sphx_world* w); /* explicit download into the host world */
/* sphx_append / sphx_remove on the solver's device state, for a caller that holds the solver object: no re-upload follows, ids survive.
 * Afterwards the host world has the device's particle count; with sync_world != 0 its arrays are downloaded and current, with 0 they are
 * marked as behind the device (as after a step with sync_world = 0).  SPHX_ERR_NOT_READY before the solver's first step and when the
 * caller has edited the world's particles since the last step (that edit is waiting for an upload: step first);
 * SPHX_ERR_INVALID_ARGUMENT on the multi-GPU solver. */
int sphx_solver_append(sphx_solver* s, sphx_world* w, const float* pos_xy, const float* vel_xy, uint32_t m, int sync_world, uint32_t* out_first_id);
int sphx_solver_remove(sphx_solver* s, sphx_world* w, const sphx_rect* rects, uint32_t n_rects, uint32_t flags, int sync_world, uint32_t* out_removed);
/* A run behind the solver object, put down and picked up: ONE file holding an 80-byte header ("SPHXSOLV", version, endianness tag, the
 * blob's size, the sphx_timer_state of t) and the context's blob (sphx_state_save).  sphx_solver_save: SPHX_ERR_NOT_READY before the
 * solver's first step and when the caller has edited the world's particles since the last step (the device does not hold that world yet).
 * sphx_solver_load: the file is validated as a whole before anything changes (sphx_state_load's rules; the timer state too); afterwards t
 * holds the saved timer state, the host world the saved boundary (caller order) and the device's particle count; its particle arrays are
 * marked as behind the device (as after a step with sync_world = 0: sphx_solver_sync_world fetches them) and the next
 * sphx_solver_simulation_step uploads nothing.  The world's fluid properties are not in the file: load into a world created like the saved
 * one (the params check refuses a context that differs).  SPHX_ERR_INVALID_ARGUMENT on the multi-GPU solver and for I/O failures. */
int sphx_solver_save(sphx_solver* s, sphx_world* w, sphx_timer* t, const char* path);
int sphx_solver_load(sphx_solver* s, sphx_world* w, sphx_timer* t, const char* path);
/* The same for the multi-GPU solver object (sphx_solver_create_dfsph_multi), under names of their own — sphx_solver_save / _load keep
 * refusing it: ONE file holding an 80-byte header ("SPHXMCKP", version, endianness tag, the size of what follows, the sphx_timer_state of
 * t) and the part(s) of sphx_multi_state_save.  checkpoint: SPHX_ERR_NOT_READY before the solver's first step and when the caller has
 * edited the world's particles since the last step.  restore: the file is validated as a whole before anything changes
 * (sphx_multi_state_load's rules; the timer state too); afterwards t holds the saved timer state, the host world the saved boundary and the
 * run's particle count, its particle arrays marked as behind the device (sphx_solver_sync_world fetches them), and the next
 * sphx_solver_simulation_step uploads nothing.  SPHX_ERR_INVALID_ARGUMENT on every other solver and for I/O failures. */
int sphx_solver_multi_checkpoint(sphx_solver* s, sphx_world* w, sphx_timer* t, const char* path);
int sphx_solver_multi_restore(sphx_solver* s, sphx_world* w, sphx_timer* t, const char* path);
sphx_ctx* sphx_solver_ctx(sphx_solver* s);
/* the sphx_multi behind a solver made by sphx_solver_create_dfsph_multi (borrowed: for sphx_multi_fluid_stats, sphx_multi_stats_*,
 * sphx_multi_info); NULL for every other solver */
sphx_multi* sphx_solver_multi(sphx_solver* s);
const char* sphx_solver_last_error(const sphx_solver* s);

#ifdef __cplusplus
}
#endif
#endif /* SPHX_H */
