// sphx_harness — headless driver over the C++ host mirror (sphx_host.hpp): the part of the reference app's loop that does not
// draw (main.rs:85-129 set-up, :177-196 scene, :279 `sph_solver.simulation_step(&mut fluid_world, &mut time_manager)`).
//
//   sphx_harness [--solver dfsph|wcsph] [--viscosity xsph|physical[:mu]] [--scale S | --particles N] [--steps K] [--warmup W] [--no-law] [--sync]
//                [--gauges x1,x2,... [--gauge-range lo:hi:dy] [--gauge-out FILE [--gauge-every K]]]
//                [--record DIR [--record-fps F] [--record-size WxH] [--record-min-pixel-radius P]]
//                [--emit x,y,w,h[:every=K][:until=S][:vel=vx,vy]] [--drain x0,y0,x1,y1]... [--keep x0,y0,x1,y1]...
//                [--load-state FILE] [--save-state FILE[:at=STEP]] [--track ID[,ID...] [--track-every E] --track-out FILE] [--fields-out FILE]
//                [--stats-out FILE [--stats-every K]]
//                [--contour-out FILE [--contour-grid x0,y0,dx,dy,nx,ny] [--contour-iso V]]
//                [--query-out FILE --query-points x,y[;x,y...] [--query-radius R]] [--select-out FILE --select x0,y0,x1,y1]
//                [--help]
//
// --query-out: after the last step, the fluid particles within R (default: the smoothing length, the largest allowed) of each of the
// --query-points in the final state (sphx_query_radius) as the CSV "point,slot,id,dist_sq": one line per entry, point after point in the
// order given, within a point in ascending slot (%.9g, which round-trips fp32).  The JSON line gains "query_entries".
// --select-out: after the last step, the fluid particles of the final state inside the --select rectangle (sphx_select; bounds may be
// inf / -inf) as the CSV "slot,id" in ascending slot.  The JSON line gains "selected".
//
// --contour-out: after the last step, the free surface of the final state (sphx_surface_contour of the fluid fraction, Wendland kernel, at
// V = 0.5 unless --contour-iso says otherwise; stitched by sphx_contour_chain) as the CSV "line,closed,x,y": the points of line 0, then of
// line 1, ... (%.9g, which round-trips fp32; a closed line repeats its first point as its last).  --contour-grid gives the lattice (fp32
// origin and spacing, whole numbers of nodes); the default is 513 x 385 nodes over the app's camera rectangle, Rect(-0.1, -0.1, 2.1, 1.6) x
// scale.  The JSON line gains "contour_segments" and "contour_lines".
//
// --stats-out: the statistics of the whole fluid (sphx_fluid_stats, record 0) are recorded on the device behind every K-th step of the
// run (sphx_stats_record; --stats-every K, default 1; warm-up and timed steps counted together) and written after the run, one JSON
// object per line and frame: step, dt, n and the members of sphx_stats_rec (%.17g, which round-trips float64).  The JSON line of the
// run gains "stats_frames".
//
// --fields-out: after the last step, the per-particle flow fields of the final state (sphx_particle_fields: velocity divergence, vorticity
// and the colour-field gradient, from the solver's own neighbour lists) as the CSV "id,x,y,divergence,vorticity,cx,cy", one line per
// particle in device order (%.9g, which round-trips fp32).  The JSON line gains "fields_particles".
//
// --track: the particles with these ids (at most SPHX_TRACK_MAX_IDS) are followed on the device (sphx_track_set + sphx_track_record): a
// frame {x, y, vx, vy} per id behind every E-th step (default 1; warm-up and timed steps counted together), nothing downloaded during the
// run.  After the run --track-out FILE receives the CSV "frame,id,x,y,vx,vy" (one line per frame and id, in the order given; %.9g, which
// round-trips fp32; "nan" for an id no particle carries at that time).  The JSON line gains "track_frames".
//
// --load-state / --save-state: the run picked up from and put down into a solver state file (sphx_solver_load / sphx_solver_save: the
// context's blob and the timer's state).  --load-state FILE starts from the file instead of the scene (solver kind, viscosity and scale
// must be those of the run that saved it: the params check refuses anything else); steps are then counted from 0 again.  --save-state FILE
// writes the file after the last step, --save-state FILE:at=STEP after STEP steps of this run (warm-up and timed steps counted together).
// A run of K steps, and a run of J < K steps that saves followed by a run that loads and does K - J steps, end in the same bits.
//
// --emit / --drain / --keep: fluid added and removed on the device between the steps (sphx_append / sphx_remove through the solver
// object).  Steps are counted from 0 over warm-up and timed steps together; the edits come before a step, from step 1 on (step 0 uploads
// the scene).  --emit appends the block add_fluid_rect(x, y, w, h, 0) makes, with velocity (vx, vy) (default 0), before every K-th step
// (default 1) below step S (default: all).  --drain removes what is inside its rectangle, --keep what is outside all --keep rectangles,
// before every step; bounds may be inf / -inf, both options may repeat, 8 rectangles in total.  The JSON line gains "emitted", "drained"
// and "final_particles" (= particles + emitted - drained).
//
// --viscosity: the solver's ViscosityModel (main.rs:93-100): XSPH (default) or PhysicalViscosityModel with fluid_viscosity mu
// (default 1.0016e-3, physical.rs:14; main.rs:96 sets 0.01).
//
// --gauges: after the run, the free-surface elevation at each x (sphx_sample_grid of the fluid fraction on a one-column lattice from lo
// in steps of dy up to hi, the rule of yasph2d_amd.gauge_elevation): "gauge_elevations": [...] in the JSON line, null where a column
// holds no fluid.  Default range lo = 0, hi = 2.5 * scale (the top of the scene), dy = particle_radius / 2.
//
// --gauge-out (needs --gauges): the same columns (x, from lo in steps of dy, floor((hi - lo) / dy) + 1 samples) are recorded on the device as
// gauges behind every K-th step of the run (sphx_probe_record of the fluid fraction at 0.5, Wendland kernel; --gauge-every K, default 1;
// warm-up and timed steps counted together) and written after the run as the CSV "step,dt,gauge,first,last,inside,x,y": one line per
// frame and gauge, the members of sphx_gauge_rec (%.9g, which round-trips fp32; "nan" for a column without fluid, first / last then
// 4294967295).  The JSON line gains "gauge_frames".  "gauge_elevations" is not affected.
//
// --record: the reference's recording mode (main.rs:310-331, :344-346, :380-397).  The timer gets TargetFrameLength(1 / F) (F = 60), the
// camera is the app's (main.rs:137: Rect(-0.1, -0.1, 2.1, 1.6) x scale fitted to a W x H screen, 1920x1080), and every completed frame is
// drawn on the device (sphx_render) and written as DIR/<frame>.ppm (binary P6, alpha dropped).  Before each step (warm-up steps included),
// frame k = 1, 2, ... is written while k / F - total_simulated_time < simulation_step: CaughtUpWithRenderTime of timemanager.rs:212-228
// with force_frame_delta(1 / F).  The accepted-lag and max_simulated_time_per_frame terms of that loop only matter against a wall
// clock and are left out; the run still ends after --steps steps.  The JSON line gains "frames": n and "last_frame_fnv" (FNV-1a of the
// last RGBA image).  --record-min-pixel-radius: sphx_render_view.min_pixel_radius (0: the reference's discs).
//
// Prints one JSON line: particle-steps/s over the K timed steps, the timer's final step, iteration statistics and an FNV-1a
// checksum of the final (downloaded) positions/velocities, which tests compare with the Python-driven run of the same scene.
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include <sys/stat.h>

#include "sphx_host.hpp"

static uint64_t fnv1a(const void* data, size_t n, uint64_t h = 1469598103934665603ull) {
    const unsigned char* p = (const unsigned char*)data;
    for (size_t i = 0; i < n; ++i) {
        h ^= p[i];
        h *= 1099511628211ull;
    }
    return h;
}

// the whole string as a finite number (a typo must not become 0)
static bool parse_double(const std::string& s, double* out) {
    char* end = nullptr;
    *out = std::strtod(s.c_str(), &end);
    return !s.empty() && end == s.c_str() + s.size() && std::isfinite(*out);
}

// Free-surface elevation of one gauge (yasph2d_amd.gauge_elevation): the fluid fraction on the lattice column y_k = fl(lo + fl(k * dy)),
// k < ny = floor((hi - lo) / dy) + 1; the highest sample with fraction >= 0.5, interpolated linearly (float64) to 0.5 towards the
// sample above it; NaN without such a sample.  Returns false when the query fails.
static bool gauge_elevation(sph::HipDfsphSolver& solver, double x, double lo, double hi, double dy, double* out) {
    const long ny = (long)std::floor((hi - lo) / dy) + 1;
    if (ny <= 0 || ny >= (1l << 31)) return false;
    std::vector<float> f((size_t)ny);
    sphx_sample_out o{};
    o.fraction = f.data();
    if (solver.sample_grid((float)x, (float)lo, 1.0f, (float)dy, 1u, (uint32_t)ny, SPHX_KERNEL_WENDLAND_C2, 0u, &o) != SPHX_OK) return false;
    auto y_of = [&](long k) { return (double)((float)lo + (float)k * (float)dy); };
    long k = ny - 1;
    while (k >= 0 && !(f[(size_t)k] >= 0.5f)) --k;
    if (k < 0)
        *out = NAN;
    else if (k == ny - 1)
        *out = y_of(k);
    else {
        const double fk = f[(size_t)k], fk1 = f[(size_t)k + 1];
        *out = y_of(k) + (fk - 0.5) / (fk - fk1) * (y_of(k + 1) - y_of(k));
    }
    return true;
}

// `count` comma-separated numbers; a rectangle bound may be infinite, never NaN
static const char* const USAGE =
    "sphx_harness [--solver dfsph|wcsph] [--viscosity xsph|physical[:mu]] [--scale S | --particles N] [--steps K] [--warmup W] [--no-law] [--sync]\n"
    "             [--gauges x1,x2,... [--gauge-range lo:hi:dy] [--gauge-out FILE [--gauge-every K]]]\n"
    "             [--record DIR [--record-fps F] [--record-size WxH] [--record-min-pixel-radius P]]\n"
    "             [--emit x,y,w,h[:every=K][:until=S][:vel=vx,vy]] [--drain x0,y0,x1,y1]... [--keep x0,y0,x1,y1]...\n"
    "             [--load-state FILE] [--save-state FILE[:at=STEP]] [--track ID[,ID...] [--track-every E] --track-out FILE] [--fields-out FILE]\n"
    "             [--stats-out FILE [--stats-every K]]\n"
    "             [--contour-out FILE [--contour-grid x0,y0,dx,dy,nx,ny] [--contour-iso V]]\n"
    "             [--query-out FILE --query-points x,y[;x,y...] [--query-radius R]] [--select-out FILE --select x0,y0,x1,y1]\n"
    "             [--help]\n"
    "  --load-state FILE            start from a solver state file (sphx_solver_load) instead of the scene\n"
    "  --save-state FILE[:at=STEP]  write a solver state file (sphx_solver_save) after STEP steps of this run; default: after the last step\n"
    "  --track ID[,ID...]           follow these particle ids on the device (sphx_track_set + sphx_track_record), a frame behind every step\n"
    "  --track-every E              ... behind every E-th step only (default 1)\n"
    "  --track-out FILE             write the frames after the run as CSV: frame,id,x,y,vx,vy\n"
    "  --gauge-out FILE             record the --gauges columns as gauges (sphx_probe_record) behind every step, write the CSV step,dt,gauge,first,last,inside,x,y\n"
    "  --gauge-every K              ... behind every K-th step\n"
    "  --stats-out FILE             record the whole fluid's statistics (sphx_stats_record) behind every step, write one JSON line per frame\n"
    "  --stats-every K              ... behind every K-th step only (default 1)\n"
    "  --fields-out FILE            write the final state's flow fields (sphx_particle_fields) as CSV: id,x,y,divergence,vorticity,cx,cy\n"
    "  --contour-out FILE           write the final state's free surface (sphx_surface_contour + sphx_contour_chain) as CSV: line,closed,x,y\n"
    "  --contour-grid x0,y0,dx,dy,nx,ny  ... on this lattice (default: 513 x 385 nodes over the camera rectangle of the scene)\n"
    "  --contour-iso V              ... at fraction V (default 0.5)\n"
    "  --query-out FILE             write the final state's fluid particles around the query points (sphx_query_radius) as CSV: point,slot,id,dist_sq\n"
    "  --query-points x,y[;x,y...]  ... the points\n"
    "  --query-radius R             ... within R (default and largest: the smoothing length)\n"
    "  --select-out FILE            write the final state's fluid particles inside a rectangle (sphx_select) as CSV: slot,id\n"
    "  --select x0,y0,x1,y1         ... the rectangle (inf allowed)\n"
    "Prints one JSON line with the throughput, the timer's final step and a checksum of the final state.\n";

static bool parse_list(const std::string& s, size_t count, bool allow_inf, double* out) {
    size_t p = 0;
    for (size_t k = 0; k < count; ++k) {
        const size_t q = std::min(s.find(',', p), s.size());
        if (k + 1 < count && q == s.size()) return false;
        const std::string t = k + 1 == count ? s.substr(p) : s.substr(p, q - p);
        char* end = nullptr;
        out[k] = std::strtod(t.c_str(), &end);
        if (t.empty() || end != t.c_str() + t.size() || std::isnan(out[k]) || (!allow_inf && !std::isfinite(out[k]))) return false;
        p = q + 1;
    }
    return true;
}

int main(int argc, char** argv) {
    std::string solver_kind = "dfsph";
    float scale = 1.0f;
    long steps = 100, warmup = 5;
    bool law = true, sync = false;
    std::string viscosity = "xsph";
    std::string gauges_arg, gauge_range_arg;
    bool want_gauges = false, want_range = false;
    std::string record_dir, record_fps_arg, record_size_arg, record_mpr_arg;
    bool want_record = false, want_fps = false, want_size = false, want_mpr = false;
    std::string emit_arg;
    bool want_emit = false;
    std::vector<sphx_rect> drain_rects, keep_rects;
    std::string load_state, save_state;
    bool want_load = false, want_save = false;
    long save_at = -1;  // (-1: after the last step)
    std::string track_arg, track_every_arg, track_out;
    bool want_track = false, want_track_every = false, want_track_out = false;
    std::string gauge_out, gauge_every_arg;
    bool want_gauge_out = false, want_gauge_every = false;
    std::string stats_out, stats_every_arg;
    bool want_stats = false, want_stats_every = false;
    std::string fields_out;
    bool want_fields = false;
    std::string contour_out, contour_grid_arg, contour_iso_arg;
    bool want_contour = false, want_contour_grid = false, want_contour_iso = false;
    std::string query_out, query_points_arg, query_radius_arg, select_out, select_arg;
    bool want_query = false, want_query_points = false, want_query_radius = false, want_select_out = false, want_select = false;
    auto add_rect = [&](std::vector<sphx_rect>& to, const char* opt, const std::string& arg) {
        double v[4];
        if (!parse_list(arg, 4, true, v) || drain_rects.size() + keep_rects.size() >= SPHX_REMOVE_MAX_RECTS) {
            std::fprintf(stderr, "invalid %s %s (x0,y0,x1,y1; inf allowed; at most %d rectangles in --drain and --keep together)\n", opt, arg.c_str(),
                         SPHX_REMOVE_MAX_RECTS);
            std::exit(2);
        }
        to.push_back(sphx_rect{(float)v[0], (float)v[1], (float)v[2], (float)v[3]});
    };
    for (int a = 1; a < argc; ++a) {
        const std::string s = argv[a];
        auto next = [&]() -> const char* { return a + 1 < argc ? argv[++a] : "0"; };
        if (s == "--solver") solver_kind = next();
        else if (s == "--viscosity") viscosity = next();
        else if (s == "--scale") scale = (float)std::atof(next());
        else if (s == "--particles") scale = (float)std::sqrt(std::atof(next()) / 4050.0);
        else if (s == "--steps") steps = std::atol(next());
        else if (s == "--warmup") warmup = std::atol(next());
        else if (s == "--no-law") law = false;
        else if (s == "--sync") sync = true;
        else if (s == "--gauges") gauges_arg = next(), want_gauges = true;
        else if (s == "--gauge-range") gauge_range_arg = next(), want_range = true;
        else if (s == "--record") record_dir = a + 1 < argc ? argv[++a] : "", want_record = true;
        else if (s == "--record-fps") record_fps_arg = next(), want_fps = true;
        else if (s == "--record-size") record_size_arg = next(), want_size = true;
        else if (s == "--record-min-pixel-radius") record_mpr_arg = next(), want_mpr = true;
        else if (s == "--emit") emit_arg = next(), want_emit = true;
        else if (s == "--drain") add_rect(drain_rects, "--drain", next());
        else if (s == "--keep") add_rect(keep_rects, "--keep", next());
        else if (s == "--load-state") load_state = a + 1 < argc ? argv[++a] : "", want_load = true;
        else if (s == "--save-state") save_state = a + 1 < argc ? argv[++a] : "", want_save = true;
        else if (s == "--track") track_arg = a + 1 < argc ? argv[++a] : "", want_track = true;
        else if (s == "--track-every") track_every_arg = next(), want_track_every = true;
        else if (s == "--track-out") track_out = a + 1 < argc ? argv[++a] : "", want_track_out = true;
        else if (s == "--gauge-out") gauge_out = a + 1 < argc ? argv[++a] : "", want_gauge_out = true;
        else if (s == "--gauge-every") gauge_every_arg = next(), want_gauge_every = true;
        else if (s == "--stats-out") stats_out = a + 1 < argc ? argv[++a] : "", want_stats = true;
        else if (s == "--stats-every") stats_every_arg = next(), want_stats_every = true;
        else if (s == "--fields-out") fields_out = a + 1 < argc ? argv[++a] : "", want_fields = true;
        else if (s == "--contour-out") contour_out = a + 1 < argc ? argv[++a] : "", want_contour = true;
        else if (s == "--contour-grid") contour_grid_arg = next(), want_contour_grid = true;
        else if (s == "--contour-iso") contour_iso_arg = next(), want_contour_iso = true;
        else if (s == "--query-out") query_out = a + 1 < argc ? argv[++a] : "", want_query = true;
        else if (s == "--query-points") query_points_arg = a + 1 < argc ? argv[++a] : "", want_query_points = true;
        else if (s == "--query-radius") query_radius_arg = next(), want_query_radius = true;
        else if (s == "--select-out") select_out = a + 1 < argc ? argv[++a] : "", want_select_out = true;
        else if (s == "--select") select_arg = a + 1 < argc ? argv[++a] : "", want_select = true;
        else if (s == "--help" || s == "-h") {
            std::fputs(USAGE, stdout);
            return 0;
        }
        else {
            std::fprintf(stderr, "unknown argument %s\n", s.c_str());
            return 2;
        }
    }
    if (want_save) {
        const size_t at = save_state.rfind(":at=");
        bool ok = true;
        if (at != std::string::npos) {
            double num;
            ok = parse_double(save_state.substr(at + 4), &num) && num >= 0.0 && num == std::floor(num) && num < 1e15;
            save_at = ok ? (long)num : -1;
            save_state.erase(at);
        }
        if (!ok || save_state.empty()) {
            std::fprintf(stderr, "invalid --save-state (FILE[:at=STEP], STEP a whole number >= 0)\n");
            return 2;
        }
    }
    if (want_load && load_state.empty()) {
        std::fprintf(stderr, "invalid --load-state (FILE)\n");
        return 2;
    }
    if (want_fields && fields_out.empty()) {
        std::fprintf(stderr, "invalid --fields-out (FILE)\n");
        return 2;
    }
    double contour_grid[6] = {0, 0, 0, 0, 0, 0}, contour_iso = 0.5;
    if (want_contour || want_contour_grid || want_contour_iso) {
        bool ok = want_contour && !contour_out.empty();
        if (ok && want_contour_grid)
            ok = parse_list(contour_grid_arg, 6, false, contour_grid) && contour_grid[2] > 0.0 && contour_grid[3] > 0.0 && contour_grid[4] >= 0.0 &&
                 contour_grid[5] >= 0.0 && contour_grid[4] == std::floor(contour_grid[4]) && contour_grid[5] == std::floor(contour_grid[5]) &&
                 contour_grid[4] * contour_grid[5] < 2147483648.0;
        if (ok && want_contour_iso) ok = parse_double(contour_iso_arg, &contour_iso);
        if (!ok) {
            std::fprintf(stderr, "invalid --contour options (--contour-out FILE [--contour-grid x0,y0,dx,dy,nx,ny: finite, dx, dy > 0, nx, ny whole numbers, "
                                 "nx * ny < 2^31] [--contour-iso V: finite])\n");
            return 2;
        }
    }
    std::vector<float> query_xy;
    double query_radius = 0.0;  // (0: the smoothing length)
    if (want_query || want_query_points || want_query_radius) {
        bool ok = want_query && !query_out.empty() && want_query_points && !query_points_arg.empty();
        for (size_t p = 0; ok && p <= query_points_arg.size();) {
            const size_t q = std::min(query_points_arg.find(';', p), query_points_arg.size());
            double v[2] = {0.0, 0.0};
            ok = parse_list(query_points_arg.substr(p, q - p), 2, false, v);
            query_xy.push_back((float)v[0]);
            query_xy.push_back((float)v[1]);
            p = q + 1;
        }
        if (ok && want_query_radius) ok = parse_double(query_radius_arg, &query_radius) && query_radius > 0.0;
        if (!ok) {
            std::fprintf(stderr, "invalid --query options (--query-out FILE --query-points x,y[;x,y...]: finite [--query-radius R: finite, > 0])\n");
            return 2;
        }
    }
    sphx_rect select_rect{0.0f, 0.0f, 0.0f, 0.0f};
    if (want_select_out || want_select) {
        double v[4] = {0.0, 0.0, 0.0, 0.0};
        const bool ok = want_select_out && !select_out.empty() && want_select && parse_list(select_arg, 4, true, v);
        if (!ok) {
            std::fprintf(stderr, "invalid --select options (--select-out FILE --select x0,y0,x1,y1; inf allowed)\n");
            return 2;
        }
        select_rect = sphx_rect{(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
    }
    uint32_t stats_every = 1;
    if (want_stats || want_stats_every) {
        double e = 1.0;
        const bool ok = want_stats && !stats_out.empty() && (!want_stats_every || (parse_double(stats_every_arg, &e) && e >= 1.0 && e == std::floor(e) && e <= 4294967295.0));
        if (!ok) {
            std::fprintf(stderr, "invalid --stats options (--stats-out FILE [--stats-every K >= 1])\n");
            return 2;
        }
        stats_every = (uint32_t)e;
    }
    std::vector<uint32_t> track_ids;
    uint32_t track_every = 1;
    if (want_track || want_track_every || want_track_out) {
        bool ok = want_track && want_track_out && !track_arg.empty() && !track_out.empty();
        for (size_t p = 0; ok && p <= track_arg.size();) {
            const size_t q = std::min(track_arg.find(',', p), track_arg.size());
            double v;
            ok = parse_double(track_arg.substr(p, q - p), &v) && v >= 0.0 && v <= 4294967295.0 && v == std::floor(v) && track_ids.size() < SPHX_TRACK_MAX_IDS;
            track_ids.push_back(ok ? (uint32_t)v : 0u);
            p = q + 1;
        }
        double e = 1.0;
        if (ok && want_track_every) ok = parse_double(track_every_arg, &e) && e >= 1.0 && e == std::floor(e) && e <= 4294967295.0;
        track_every = (uint32_t)e;
        if (!ok) {
            std::fprintf(stderr, "invalid --track options (--track ID[,ID...] with at most %d whole numbers < 2^32, [--track-every E >= 1], --track-out FILE)\n",
                         SPHX_TRACK_MAX_IDS);
            return 2;
        }
    }
    const bool wcsph = solver_kind == "wcsph";
    sph::FluidParticleWorld world(2.0f, 10000.0f, 100.0f);  // main.rs:85-89
    sph::reset_fluid(world, scale);                          // main.rs:177-196
    std::vector<double> gauge_x;
    double gauge_lo = 0.0, gauge_hi = 2.5 * (double)scale, gauge_dy = (double)world.properties.particle_radius() / 2.0;
    if (want_gauges) {
        bool ok = !gauges_arg.empty();
        for (size_t p = 0; ok && p <= gauges_arg.size();) {
            const size_t q = std::min(gauges_arg.find(',', p), gauges_arg.size());
            double v;
            ok = parse_double(gauges_arg.substr(p, q - p), &v);
            gauge_x.push_back(v);
            p = q + 1;
        }
        if (!ok) {
            std::fprintf(stderr, "invalid --gauges %s (x1,x2,... finite numbers)\n", gauges_arg.c_str());
            return 2;
        }
    }
    if (want_range) {
        const size_t c1 = gauge_range_arg.find(':'), c2 = c1 == std::string::npos ? c1 : gauge_range_arg.find(':', c1 + 1);
        bool ok = want_gauges && c2 != std::string::npos && gauge_range_arg.find(':', c2 + 1) == std::string::npos &&
                  parse_double(gauge_range_arg.substr(0, c1), &gauge_lo) && parse_double(gauge_range_arg.substr(c1 + 1, c2 - c1 - 1), &gauge_hi) &&
                  parse_double(gauge_range_arg.substr(c2 + 1), &gauge_dy) && gauge_dy > 0.0 && gauge_hi >= gauge_lo &&
                  (gauge_hi - gauge_lo) / gauge_dy < 2147483647.0;
        if (!ok) {
            std::fprintf(stderr, "invalid --gauge-range %s (lo:hi:dy, finite, lo <= hi, dy > 0, with --gauges)\n", gauge_range_arg.c_str());
            return 2;
        }
    }
    uint32_t gauge_every = 1;
    std::vector<sphx_gauge> gauge_rays;  // the --gauges columns as gauges (--gauge-out)
    if (want_gauge_out || want_gauge_every) {
        double e = 1.0;
        const double ny = std::floor((gauge_hi - gauge_lo) / gauge_dy) + 1.0;
        const bool ok = want_gauge_out && want_gauges && !gauge_out.empty() && gauge_x.size() <= SPHX_GAUGE_MAX && ny >= 1.0 && ny <= 1048576.0 &&
                        (!want_gauge_every || (parse_double(gauge_every_arg, &e) && e >= 1.0 && e == std::floor(e) && e <= 4294967295.0));
        if (!ok) {
            std::fprintf(stderr, "invalid --gauge options (--gauge-out FILE [--gauge-every K >= 1], with --gauges of at most %d columns of at most 2^20 samples)\n",
                         SPHX_GAUGE_MAX);
            return 2;
        }
        gauge_every = (uint32_t)e;
        for (double x : gauge_x) gauge_rays.push_back(sphx_gauge{(float)x, (float)gauge_lo, 0.0f, (float)gauge_dy, (uint32_t)ny, {0u, 0u, 0u}});
    }
    double record_fps = 60.0, record_mpr = 0.0;
    uint32_t record_w = 1920, record_h = 1080;
    if (want_record || want_fps || want_size || want_mpr) {
        bool ok = want_record && !record_dir.empty();
        if (ok && want_fps) ok = parse_double(record_fps_arg, &record_fps) && record_fps > 0.0 && record_fps <= 1e9;
        if (ok && want_mpr) ok = parse_double(record_mpr_arg, &record_mpr) && record_mpr >= 0.0 && record_mpr <= 4.0;
        if (ok && want_size) {
            const size_t x = record_size_arg.find('x');
            double w = 0, h = 0;
            ok = x != std::string::npos && parse_double(record_size_arg.substr(0, x), &w) && parse_double(record_size_arg.substr(x + 1), &h) &&
                 w >= 1.0 && h >= 1.0 && w == std::floor(w) && h == std::floor(h) && w * h < 268435456.0;
            record_w = ok ? (uint32_t)w : 0u, record_h = ok ? (uint32_t)h : 0u;
        }
        if (!ok) {
            std::fprintf(stderr, "invalid --record options (--record DIR [--record-fps F > 0] [--record-size WxH, W * H < 2^28] "
                                 "[--record-min-pixel-radius P in [0, 4]])\n");
            return 2;
        }
    }
    std::vector<sph::Point> emit_pos;
    std::vector<sph::Vector> emit_vel;
    long emit_every = 1, emit_until = -1;
    if (want_emit) {
        double r[4], vel[2] = {0.0, 0.0}, num;
        bool ok = true;
        size_t p = std::min(emit_arg.find(':'), emit_arg.size());
        ok = parse_list(emit_arg.substr(0, p), 4, false, r) && r[2] > 0.0 && r[3] > 0.0;
        while (ok && p < emit_arg.size()) {
            const size_t q = std::min(emit_arg.find(':', p + 1), emit_arg.size());
            const std::string opt = emit_arg.substr(p + 1, q - p - 1);
            if (opt.rfind("every=", 0) == 0) ok = parse_double(opt.substr(6), &num) && num >= 1.0 && num == std::floor(num) && num < 1e9, emit_every = ok ? (long)num : 1;
            else if (opt.rfind("until=", 0) == 0) ok = parse_double(opt.substr(6), &num) && num >= 0.0 && num == std::floor(num) && num < 1e15, emit_until = ok ? (long)num : -1;
            else if (opt.rfind("vel=", 0) == 0) ok = parse_list(opt.substr(4), 2, false, vel);
            else ok = false;
            p = q;
        }
        if (!ok) {
            std::fprintf(stderr, "invalid --emit %s (x,y,w,h[:every=K][:until=S][:vel=vx,vy], finite, w, h > 0, K >= 1)\n", emit_arg.c_str());
            return 2;
        }
        sph::FluidParticleWorld block(2.0f, 10000.0f, 100.0f);
        block.add_fluid_rect((float)r[0], (float)r[1], (float)r[2], (float)r[3], 0.0f);
        emit_pos = block.particles.positions;
        emit_vel.assign(emit_pos.size(), sph::Vector{(float)vel[0], (float)vel[1]});
    }
    const bool want_edit = want_emit || !drain_rects.empty() || !keep_rects.empty();
    sphx_params params = sph::HipDfsphSolver::params_of(world, nullptr);
    {
        const size_t colon = viscosity.find(':');
        const std::string model = viscosity.substr(0, colon);
        bool ok = model == "xsph" ? colon == std::string::npos : model == "physical";
        if (ok && model == "physical") {
            params.viscosity_model = SPHX_VISCOSITY_PHYSICAL;
            if (colon != std::string::npos) {  // the whole rest must be a number: a typo must not become mu = 0 (an inviscid run)
                const char* s = viscosity.c_str() + colon + 1;
                char* end = nullptr;
                params.fluid_viscosity = std::strtof(s, &end);
                ok = end != s && *end == '\0' && std::isfinite(params.fluid_viscosity);
            }
        }
        if (!ok) {
            std::fprintf(stderr, "invalid --viscosity %s (xsph | physical[:mu], mu a finite number)\n", viscosity.c_str());
            return 2;
        }
    }
    std::unique_ptr<sph::HipDfsphSolver> solver(wcsph ? new sph::HipWcsphSolver(world, &params) : new sph::HipDfsphSolver(world, &params));
    if (!solver->ok()) {
        std::fprintf(stderr, "solver: %s (status %d)\n", solver->last_error.c_str(), solver->last_status);
        return 1;  // no CPU fallback
    }
    solver->sync_every_step = sync;
    solver->use_timer_law = law;
    sph::TimeManager tm = sph::TimeManager::adaptive(sph::Duration::from_secs_f32(1.0f / 120.0f / 3.0f), sph::Duration::from_secs_f32(1.0f / 60.0f / 400.0f),
                                                     wcsph ? 0.2f : 1.5f);  // main.rs:115-127
    if (want_load && solver->load(world, tm, load_state.c_str()) != SPHX_OK) {
        std::fprintf(stderr, "--load-state %s failed: %s (status %d)\n", load_state.c_str(), solver->last_error.c_str(), solver->last_status);
        return 1;
    }
    const size_t n = world.particles.positions.size();
    // the trajectory recorder: set and recording belong to the context, the upload of step 0 leaves them alone
    const uint64_t track_max_frames = want_track ? (uint64_t)std::max(warmup + steps, 0l) / track_every : 0;
    if (track_max_frames) {
        int rc = track_max_frames > 0xFFFFFFFFull ? SPHX_ERR_CAPACITY : sphx_track_set(solver->ctx(), track_ids.data(), (uint32_t)track_ids.size());
        if (rc == SPHX_OK) rc = sphx_track_record(solver->ctx(), (uint32_t)track_max_frames, track_every);
        if (rc != SPHX_OK) {
            std::fprintf(stderr, "--track failed: %s (status %d)\n", sphx_last_error(solver->ctx()), rc);
            return 1;
        }
    }
    // the statistics recorder, likewise
    const uint64_t stats_max_frames = want_stats ? (uint64_t)std::max(warmup + steps, 0l) / stats_every : 0;
    if (stats_max_frames) {
        const int rc = stats_max_frames > 0xFFFFFFFFull ? SPHX_ERR_CAPACITY : sphx_stats_record(solver->ctx(), nullptr, 0u, (uint32_t)stats_max_frames, stats_every);
        if (rc != SPHX_OK) {
            std::fprintf(stderr, "--stats-out failed: %s (status %d)\n", sphx_last_error(solver->ctx()), rc);
            return 1;
        }
    }
    // the gauge recorder, likewise
    const uint64_t gauge_max_frames = want_gauge_out ? (uint64_t)std::max(warmup + steps, 0l) / gauge_every : 0;
    if (gauge_max_frames) {
        const int rc = gauge_max_frames > 0xFFFFFFFFull
                           ? SPHX_ERR_CAPACITY
                           : sphx_probe_record(solver->ctx(), nullptr, 0u, gauge_rays.data(), (uint32_t)gauge_rays.size(), SPHX_KERNEL_WENDLAND_C2,
                                               SPHX_GAUGE_FIELD_FRACTION, 0.5f, (uint32_t)gauge_max_frames, gauge_every);
        if (rc != SPHX_OK) {
            std::fprintf(stderr, "--gauge-out failed: %s (status %d)\n", sphx_last_error(solver->ctx()), rc);
            return 1;
        }
    }
    // recording mode
    sph::Camera camera = sph::Camera::center_around_world_rect(record_w, record_h, -0.1f * scale, -0.1f * scale, 2.1f * scale, 1.6f * scale);  // main.rs:137
    camera.view.min_pixel_radius = (float)record_mpr;
    const uint64_t frame_ns = (uint64_t)std::llround(1e9 / record_fps);  // Duration::from_secs_f64(1.0 / RECORDING_FPS)
    uint64_t frames = 0, last_frame_fnv = 0;
    std::vector<uint8_t> image;
    if (want_record) {
        tm.timestep_target_frame = sph::Duration{frame_ns};  // main.rs:323-326
        frames = tm.total_simulated_time.ns / frame_ns;      // (0 unless --load-state: the frames before the save were drawn by that run)
        mkdir(record_dir.c_str(), 0777);
        image.resize((size_t)record_w * record_h * 4);
    }
    auto record_due_frames = [&]() {
        for (;;) {
            const uint64_t due = (frames + 1) * frame_ns, done = tm.total_simulated_time.ns;
            if ((due > done ? due - done : 0) >= tm.simulation_step().ns) return;  // PerformStepAndCallAgain
            // frame `frames + 1` is complete: draw it
            sphx_render_out o{image.data(), nullptr};
            const int rc = solver->render(camera, 0u, &o);
            if (rc != SPHX_OK) {
                std::fprintf(stderr, "render failed: %s (status %d)\n", sphx_last_error(solver->ctx()), rc);
                std::exit(1);
            }
            ++frames;
            last_frame_fnv = fnv1a(image.data(), image.size());
            const std::string path = record_dir + "/" + std::to_string(frames) + ".ppm";
            FILE* f = std::fopen(path.c_str(), "wb");
            bool ok = f != nullptr;
            if (ok) {
                std::vector<uint8_t> rgb((size_t)record_w * record_h * 3);
                for (size_t p = 0; p < (size_t)record_w * record_h; ++p) std::memcpy(&rgb[3 * p], &image[4 * p], 3);
                ok = std::fprintf(f, "P6\n%u %u\n255\n", record_w, record_h) > 0 && std::fwrite(rgb.data(), 1, rgb.size(), f) == rgb.size();
                ok = std::fclose(f) == 0 && ok;
            }
            if (!ok) {
                std::fprintf(stderr, "cannot write %s\n", path.c_str());
                std::exit(1);
            }
        }
    };
    unsigned long long emitted = 0, drained = 0;
    long step_index = 0;
    auto edit = [&]() {  // before step `step_index` (>= 1: the device holds the scene)
        auto check = [&](int rc, const char* what) {
            if (rc != SPHX_OK) {
                std::fprintf(stderr, "%s failed: %s (status %d)\n", what, solver->last_error.c_str(), rc);
                std::exit(1);
            }
        };
        if (want_emit && !emit_pos.empty() && step_index % emit_every == 0 && (emit_until < 0 || step_index < emit_until)) {
            check(solver->append(world, &emit_pos[0].x, &emit_vel[0].x, (uint32_t)emit_pos.size(), sync, nullptr), "--emit");
            emitted += emit_pos.size();
        }
        uint32_t gone = 0;
        if (!drain_rects.empty()) {
            check(solver->remove(world, drain_rects.data(), (uint32_t)drain_rects.size(), 0u, sync, &gone), "--drain");
            drained += gone;
        }
        if (!keep_rects.empty()) {
            check(solver->remove(world, keep_rects.data(), (uint32_t)keep_rects.size(), SPHX_REMOVE_OUTSIDE, sync, &gone), "--keep");
            drained += gone;
        }
    };
    auto save = [&]() {
        if (solver->save(world, tm, save_state.c_str()) != SPHX_OK) {
            std::fprintf(stderr, "--save-state %s failed: %s (status %d)\n", save_state.c_str(), solver->last_error.c_str(), solver->last_status);
            std::exit(1);
        }
    };
    if (want_save && save_at == 0) save();  // (only a loaded run holds a state before its first step)
    auto step = [&]() {
        if (want_edit && step_index > 0) edit();
        ++step_index;
        if (want_record) record_due_frames();
        tm.on_step_started();
        solver->simulation_step(world, tm);
        if (solver->last_status != SPHX_OK) {
            std::fprintf(stderr, "step failed: %s (status %d)\n", solver->last_error.c_str(), solver->last_status);
            std::exit(1);
        }
        if (want_save && step_index == save_at) save();
    };
    for (long i = 0; i < warmup; ++i) step();
    sphx_synchronize(solver->ctx());
    unsigned long long id_sum = 0, iv_sum = 0;
    const auto t0 = std::chrono::steady_clock::now();
    for (long i = 0; i < steps; ++i) {
        step();
        id_sum += solver->last_stats.density_iterations;
        iv_sum += solver->last_stats.divergence_iterations;
    }
    sphx_synchronize(solver->ctx());
    const double el = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (want_save && save_at < 0) save();
    if (solver->sync_world(world) != SPHX_OK) return 1;
    // order-independent content check: positions/velocities placed at their persistent particle id
    const size_t n_final = world.particles.positions.size();  // (== n unless --emit / --drain / --keep edited the set; ids < n + emitted)
    size_t id_span = n + emitted;
    if (want_load)  // (a loaded set may hold ids of particles that were appended and removed before the save)
        for (size_t i = 0; i < n_final; ++i) id_span = std::max<size_t>(id_span, (size_t)world.particles.particle_ids[i] + 1);
    std::vector<float> by_id(4 * id_span, 0.0f);
    for (size_t i = 0; i < n_final; ++i) {
        const uint32_t id = world.particles.particle_ids[i];
        by_id[4 * id + 0] = world.particles.positions[i].x;
        by_id[4 * id + 1] = world.particles.positions[i].y;
        by_id[4 * id + 2] = world.particles.velocities[i].x;
        by_id[4 * id + 3] = world.particles.velocities[i].y;
    }
    std::string gauge_json;  // (empty without --gauges: the line stays what it was)
    if (want_gauges) {
        gauge_json = ", \"gauge_elevations\": [";
        for (size_t g = 0; g < gauge_x.size(); ++g) {
            double e;
            if (!gauge_elevation(*solver, gauge_x[g], gauge_lo, gauge_hi, gauge_dy, &e)) {
                std::fprintf(stderr, "gauge at x = %g: %s\n", gauge_x[g], sphx_last_error(solver->ctx()));
                return 1;
            }
            char buf[64];
            if (std::isnan(e))
                std::snprintf(buf, sizeof(buf), "null");
            else
                std::snprintf(buf, sizeof(buf), "%.17g", e);
            gauge_json += (g ? ", " : "") + std::string(buf);
        }
        gauge_json += "]";
    }
    if (want_gauge_out) {
        sphx_probe_status ps{};
        std::vector<sphx_gauge_rec> rec;
        std::vector<sphx_stats_frame> info;
        int rc = sphx_probe_get_status(solver->ctx(), &ps);
        if (rc == SPHX_OK && ps.frames) {
            rec.resize((size_t)ps.frames * ps.n_gauges);
            info.resize(ps.frames);
            rc = sphx_probe_read(solver->ctx(), 0u, ps.frames, nullptr, rec.data(), info.data());
        }
        if (rc != SPHX_OK) {
            std::fprintf(stderr, "--gauge-out: %s (status %d)\n", sphx_last_error(solver->ctx()), rc);
            return 1;
        }
        FILE* f = std::fopen(gauge_out.c_str(), "w");
        bool ok = f != nullptr && std::fputs("step,dt,gauge,first,last,inside,x,y\n", f) >= 0;
        for (size_t k = 0; ok && k < rec.size(); ++k) {
            const sphx_gauge_rec& r = rec[k];
            const sphx_stats_frame& fr = info[k / ps.n_gauges];
            ok = std::fprintf(f, "%llu,%.9g,%zu,%u,%u,%u,%.9g,%.9g\n", (unsigned long long)fr.step, (double)fr.dt, k % ps.n_gauges, r.first, r.last, r.inside,
                              (double)r.x, (double)r.y) > 0;
        }
        if (f) ok = std::fclose(f) == 0 && ok;
        if (!ok) {
            std::fprintf(stderr, "cannot write %s\n", gauge_out.c_str());
            return 1;
        }
        char buf[64];
        std::snprintf(buf, sizeof(buf), ", \"gauge_frames\": %u", ps.frames);
        gauge_json += buf;
    }
    if (want_record) {
        char buf[96];
        std::snprintf(buf, sizeof(buf), ", \"frames\": %llu, \"last_frame_fnv\": \"%016llx\"", (unsigned long long)frames, (unsigned long long)last_frame_fnv);
        gauge_json += buf;
    }
    if (want_track) {
        sphx_track_status ts{};
        std::vector<float> fr;
        int rc = sphx_track_get_status(solver->ctx(), &ts);
        if (rc == SPHX_OK && ts.frames) {
            fr.resize((size_t)ts.frames * ts.m * 4);
            rc = sphx_track_read(solver->ctx(), 0u, ts.frames, 0u, fr.data());
        }
        if (rc != SPHX_OK) {
            std::fprintf(stderr, "--track-out: %s (status %d)\n", sphx_last_error(solver->ctx()), rc);
            return 1;
        }
        FILE* f = std::fopen(track_out.c_str(), "w");
        bool ok = f != nullptr && std::fputs("frame,id,x,y,vx,vy\n", f) >= 0;
        for (size_t k = 0; ok && k < (size_t)ts.frames * ts.m; ++k)
            ok = std::fprintf(f, "%zu,%u,%.9g,%.9g,%.9g,%.9g\n", k / ts.m, track_ids[k % ts.m], (double)fr[4 * k], (double)fr[4 * k + 1], (double)fr[4 * k + 2],
                              (double)fr[4 * k + 3]) > 0;
        if (f) ok = std::fclose(f) == 0 && ok;
        if (!ok) {
            std::fprintf(stderr, "cannot write %s\n", track_out.c_str());
            return 1;
        }
        char buf[64];
        std::snprintf(buf, sizeof(buf), ", \"track_frames\": %u", ts.frames);
        gauge_json += buf;
    }
    if (want_stats) {
        sphx_stats_status ss{};
        std::vector<sphx_stats_rec> rec;
        std::vector<sphx_stats_frame> info;
        int rc = sphx_stats_get_status(solver->ctx(), &ss);
        if (rc == SPHX_OK && ss.frames) {
            rec.resize(ss.frames);
            info.resize(ss.frames);
            rc = sphx_stats_read(solver->ctx(), 0u, ss.frames, rec.data(), info.data());
        }
        if (rc != SPHX_OK) {
            std::fprintf(stderr, "--stats-out: %s (status %d)\n", sphx_last_error(solver->ctx()), rc);
            return 1;
        }
        FILE* f = std::fopen(stats_out.c_str(), "w");
        bool ok = f != nullptr;
        auto num = [](double v) {  // (JSON has no inf: the extremes of an empty record are written as null)
            char b[40];
            if (std::isfinite(v)) std::snprintf(b, sizeof(b), "%.17g", v);
            else std::snprintf(b, sizeof(b), "null");
            return std::string(b);
        };
        for (size_t k = 0; ok && k < rec.size(); ++k) {
            const sphx_stats_rec& r = rec[k];
            ok = std::fprintf(f, "{\"step\": %llu, \"dt\": %.9g, \"n\": %u, \"count\": %llu, \"nonfinite\": %llu, \"density_count\": %llu, \"density_valid\": %u, "
                                 "\"sum_pos\": [%s, %s], \"sum_vel\": [%s, %s], \"sum_speed_sq\": %s, \"sum_angular\": %s, \"sum_density\": %s, "
                                 "\"sum_density_sq\": %s, \"max_speed_sq\": %s, \"min_pos\": [%s, %s], \"max_pos\": [%s, %s], \"min_density\": %s, \"max_density\": %s}\n",
                              (unsigned long long)info[k].step, (double)info[k].dt, info[k].n, (unsigned long long)r.count, (unsigned long long)r.nonfinite,
                              (unsigned long long)r.density_count, r.density_valid, num(r.sum_pos[0]).c_str(), num(r.sum_pos[1]).c_str(), num(r.sum_vel[0]).c_str(),
                              num(r.sum_vel[1]).c_str(), num(r.sum_speed_sq).c_str(), num(r.sum_angular).c_str(), num(r.sum_density).c_str(),
                              num(r.sum_density_sq).c_str(), num(r.max_speed_sq).c_str(), num(r.min_pos[0]).c_str(), num(r.min_pos[1]).c_str(),
                              num(r.max_pos[0]).c_str(), num(r.max_pos[1]).c_str(), num(r.min_density).c_str(), num(r.max_density).c_str()) > 0;
        }
        if (f) ok = std::fclose(f) == 0 && ok;
        if (!ok) {
            std::fprintf(stderr, "cannot write %s\n", stats_out.c_str());
            return 1;
        }
        char buf[64];
        std::snprintf(buf, sizeof(buf), ", \"stats_frames\": %u", ss.frames);
        gauge_json += buf;
    }
    if (want_fields) {
        std::vector<float> div(n_final), vort(n_final), cg(2 * n_final);
        sphx_fields_out fo{};
        fo.divergence = div.data();
        fo.vorticity = vort.data();
        fo.color_grad = cg.data();
        const int rc = sphx_particle_fields(solver->ctx(), 0u, &fo);
        if (rc != SPHX_OK) {
            std::fprintf(stderr, "--fields-out: %s (status %d)\n", sphx_last_error(solver->ctx()), rc);
            return 1;
        }
        FILE* f = std::fopen(fields_out.c_str(), "w");
        bool ok = f != nullptr && std::fputs("id,x,y,divergence,vorticity,cx,cy\n", f) >= 0;
        for (size_t i = 0; ok && i < n_final; ++i)
            ok = std::fprintf(f, "%u,%.9g,%.9g,%.9g,%.9g,%.9g,%.9g\n", world.particles.particle_ids[i], (double)world.particles.positions[i].x,
                              (double)world.particles.positions[i].y, (double)div[i], (double)vort[i], (double)cg[2 * i], (double)cg[2 * i + 1]) > 0;
        if (f) ok = std::fclose(f) == 0 && ok;
        if (!ok) {
            std::fprintf(stderr, "cannot write %s\n", fields_out.c_str());
            return 1;
        }
        char buf[64];
        std::snprintf(buf, sizeof(buf), ", \"fields_particles\": %zu", n_final);
        gauge_json += buf;
    }
    if (want_contour) {
        if (!want_contour_grid) {  // the app's camera rectangle (main.rs:137) x scale
            contour_grid[0] = contour_grid[1] = -0.1 * (double)scale;
            contour_grid[2] = 2.2 * (double)scale / 512.0, contour_grid[3] = 1.7 * (double)scale / 384.0;
            contour_grid[4] = 513.0, contour_grid[5] = 385.0;
        }
        const float gx0 = (float)contour_grid[0], gy0 = (float)contour_grid[1], gdx = (float)contour_grid[2], gdy = (float)contour_grid[3];
        const uint32_t gnx = (uint32_t)contour_grid[4], gny = (uint32_t)contour_grid[5];
        uint32_t total = 0, lines = 0;
        sphx_contour_out co{};
        co.count = &total;
        int rc = sphx_surface_contour(solver->ctx(), gx0, gy0, gdx, gdy, gnx, gny, SPHX_KERNEL_WENDLAND_C2, SPHX_CONTOUR_FIELD_FRACTION, (float)contour_iso, 0u, 0u, &co);
        std::vector<float> seg(4 * (size_t)total);
        if (rc == SPHX_OK && total) {
            co.segments = seg.data();
            rc = sphx_surface_contour(solver->ctx(), gx0, gy0, gdx, gdy, gnx, gny, SPHX_KERNEL_WENDLAND_C2, SPHX_CONTOUR_FIELD_FRACTION, (float)contour_iso, total, 0u, &co);
        }
        if (rc != SPHX_OK) {
            std::fprintf(stderr, "--contour-out: %s (status %d)\n", sphx_last_error(solver->ctx()), rc);
            return 1;
        }
        const uint32_t ns = (uint32_t)(seg.size() / 4);
        std::vector<uint32_t> order(ns), first((size_t)ns + 1);
        std::vector<uint8_t> closed(ns);
        if (sphx_contour_chain(seg.data(), ns, order.data(), first.data(), closed.data(), &lines) != SPHX_OK) {
            std::fprintf(stderr, "--contour-out: sphx_contour_chain failed\n");
            return 1;
        }
        FILE* f = std::fopen(contour_out.c_str(), "w");
        bool ok = f != nullptr && std::fputs("line,closed,x,y\n", f) >= 0;
        for (uint32_t k = 0; ok && k < lines; ++k) {
            const float* s0 = seg.data() + 4 * (size_t)order[first[k]];
            ok = std::fprintf(f, "%u,%u,%.9g,%.9g\n", k, (unsigned)closed[k], (double)s0[0], (double)s0[1]) > 0;
            for (uint32_t q = first[k]; ok && q < first[k + 1]; ++q) {
                const float* s = seg.data() + 4 * (size_t)order[q];
                ok = std::fprintf(f, "%u,%u,%.9g,%.9g\n", k, (unsigned)closed[k], (double)s[2], (double)s[3]) > 0;
            }
        }
        if (f) ok = std::fclose(f) == 0 && ok;
        if (!ok) {
            std::fprintf(stderr, "cannot write %s\n", contour_out.c_str());
            return 1;
        }
        char buf[96];
        std::snprintf(buf, sizeof(buf), ", \"contour_segments\": %u, \"contour_lines\": %u", total, lines);
        gauge_json += buf;
    }
    if (want_query) {
        const uint32_t qm = (uint32_t)(query_xy.size() / 2);
        const float qr = want_query_radius ? (float)query_radius : params.smoothing_length;
        uint64_t total = 0;
        std::vector<uint64_t> off((size_t)qm + 1);
        sphx_query_out qo{};
        qo.offsets = off.data();
        qo.count = &total;
        int rc = sphx_query_radius(solver->ctx(), query_xy.data(), qm, qr, 0u, 0u, &qo);
        std::vector<uint32_t> slot((size_t)total), id((size_t)total);
        std::vector<float> d2((size_t)total);
        if (rc == SPHX_OK && total) {
            qo.index = slot.data(), qo.id = id.data(), qo.dist_sq = d2.data();
            rc = sphx_query_radius(solver->ctx(), query_xy.data(), qm, qr, total, 0u, &qo);
        }
        if (rc != SPHX_OK) {
            std::fprintf(stderr, "--query-out: %s (status %d)\n", sphx_last_error(solver->ctx()), rc);
            return 1;
        }
        FILE* f = std::fopen(query_out.c_str(), "w");
        bool ok = f != nullptr && std::fputs("point,slot,id,dist_sq\n", f) >= 0;
        for (uint32_t k = 0; ok && k < qm; ++k)
            for (uint64_t e = off[k]; ok && e < off[k + 1] && e < slot.size(); ++e)
                ok = std::fprintf(f, "%u,%u,%u,%.9g\n", k, slot[e], id[e], (double)d2[e]) > 0;
        if (f) ok = std::fclose(f) == 0 && ok;
        if (!ok) {
            std::fprintf(stderr, "cannot write %s\n", query_out.c_str());
            return 1;
        }
        char buf[64];
        std::snprintf(buf, sizeof(buf), ", \"query_entries\": %llu", (unsigned long long)total);
        gauge_json += buf;
    }
    if (want_select_out) {
        uint32_t total = 0;
        sphx_select_out so{};
        so.count = &total;
        int rc = sphx_select(solver->ctx(), &select_rect, 1u, 0u, 0u, &so);
        std::vector<uint32_t> slot(total), id(total);
        if (rc == SPHX_OK && total) {
            so.index = slot.data(), so.id = id.data();
            rc = sphx_select(solver->ctx(), &select_rect, 1u, 0u, total, &so);
        }
        if (rc != SPHX_OK) {
            std::fprintf(stderr, "--select-out: %s (status %d)\n", sphx_last_error(solver->ctx()), rc);
            return 1;
        }
        FILE* f = std::fopen(select_out.c_str(), "w");
        bool ok = f != nullptr && std::fputs("slot,id\n", f) >= 0;
        for (size_t e = 0; ok && e < slot.size(); ++e) ok = std::fprintf(f, "%u,%u\n", slot[e], id[e]) > 0;
        if (f) ok = std::fclose(f) == 0 && ok;
        if (!ok) {
            std::fprintf(stderr, "cannot write %s\n", select_out.c_str());
            return 1;
        }
        char buf[64];
        std::snprintf(buf, sizeof(buf), ", \"selected\": %u", total);
        gauge_json += buf;
    }
    if (want_edit) {
        char buf[128];
        std::snprintf(buf, sizeof(buf), ", \"emitted\": %llu, \"drained\": %llu, \"final_particles\": %zu", emitted, drained, n_final);
        gauge_json += buf;
    }
    std::printf("{\"solver\": \"%s\", \"viscosity\": \"%s\", \"fluid_viscosity\": %.9g, \"particles\": %zu, \"boundary\": %zu, \"steps\": %ld, \"particle_steps_per_s\": %.6e, \"ms_per_step\": %.6f, "
                "\"timer_step_ns\": %llu, \"simulated_ns\": %llu, \"mean_density_iterations\": %.4f, \"mean_divergence_iterations\": %.4f, "
                "\"state_fnv1a\": \"%016llx\"%s}\n",
                solver_kind.c_str(), params.viscosity_model == SPHX_VISCOSITY_PHYSICAL ? "physical" : "xsph", (double)params.fluid_viscosity, n, world.particles.boundary_particles.size(), steps, (double)n * (double)steps / el, el / (double)steps * 1e3,
                (unsigned long long)tm.simulation_step().ns, (unsigned long long)tm.total_simulated_time.ns, steps ? (double)id_sum / steps : 0.0,
                steps ? (double)iv_sum / steps : 0.0, (unsigned long long)fnv1a(by_id.data(), by_id.size() * 4), gauge_json.c_str());
    return 0;
}
