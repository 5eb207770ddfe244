// sphx_launch.inc — host side of libsphx's device path: context, memory, per-phase launch sequences and the C ABI of
// include/sphx.h.  Included at the end of sphx_kernels.hip (one translation unit so the kernels are visible).
#include <algorithm>
#include <cmath>

using namespace sphx;

static std::string g_create_error;

#define SPHX_HIP(ctx, expr)                                                        \
    do {                                                                           \
        hipError_t e__ = (expr);                                                   \
        if (e__ != hipSuccess) return (ctx)->fail(SPHX_ERR_HIP, #expr, hipGetErrorString(e__)); \
    } while (0)

namespace {

// 256-thread particle kernels: the grid is rounded up to a multiple of 8 workgroups (xcd_bid() deals contiguous eighths of the
// particles to the 8 XCDs; surplus workgroups find i >= n)
inline uint32_t nblocks(uint32_t n, uint32_t per = 256) {
    const uint32_t b = (n + per - 1) / per;
    return per == 256 ? (b + 7u) & ~7u : b;
}
// mean neighbour-list length of the latest build (for the algorithmic byte counts handed to the profiler)
inline double kbar_of(const sphx_ctx* c) { return (c->N && c->nb_last) ? (double)c->nb_last / (double)c->N : 12.0; }
// algorithmic list bytes per particle and traversal: 10-bit workgroup-local entries + the 4-byte lines of the out-of-window table
// + the workgroup's table size / 256 (nearly every workgroup at the default table size), or 32-bit entries when that is off
inline double list_bytes(const sphx_ctx* c) {
    if (!c->K.remote_cap) return 2.0 + 4.0 * kbar_of(c);
    const double rbar = c->N ? (double)c->rem_last / (double)c->N : 0.5;
    // 16-bit NeighborRange word (+ a format word per wavefront), 10-bit entries three to a 32-bit word, 4-byte table lines
    return 2.0 + 4.0 / 64.0 + (4.0 / 3.0) * kbar_of(c) + 4.0 * rbar + 4.0 / 256.0;
}

// f32::powi -> compiler-rt __powisf2 (square-and-multiply); used by the kernel constructors of the reference
float rs_powi(float a, int b) {
    const bool recip = b < 0;
    float r = 1;
    for (;;) {
        if (b & 1) r *= a;
        b /= 2;
        if (b == 0) break;
        a *= a;
    }
    return recip ? 1 / r : r;
}

// ---- profiling ---------------------------------------------------------------------------------------------------
hipEvent_t prof_event(sphx_ctx* c) {
    if (!c->ev_pool.empty()) {
        hipEvent_t e = c->ev_pool.back();
        c->ev_pool.pop_back();
        return e;
    }
    hipEvent_t e;
    hipEventCreate(&e);
    return e;
}
void prof_resolve(sphx_ctx* c) {
    if (c->prof_pending.empty()) return;
    hipStreamSynchronize(c->stream);
    for (auto& p : c->prof_pending) {
        float ms = 0;
        hipEventElapsedTime(&ms, p.a, p.b);
        ProfTotals& t = c->prof_totals[p.name];
        t.launches += 1;
        t.ms += ms;
        t.bytes += p.bytes;
        c->ev_pool.push_back(p.a);
        c->ev_pool.push_back(p.b);
    }
    c->prof_pending.clear();
}
// roctx ranges named after the reference's microprofile scopes (dfsph.rs:69,100,129,..., neighborhood_search.rs:98,...): they show up
// in `rocprofv3 --marker-trace` timelines.  Off unless SPHX_ROCTX=1 (resolved with dlopen, so the library has no hard dependency).
struct Roctx {
    int (*push)(const char*) = nullptr;
    int (*pop)() = nullptr;
    Roctx() {
        const char* e = std::getenv("SPHX_ROCTX");
        if (!e || e[0] != '1') return;
        for (const char* lib : {"librocprofiler-sdk-roctx.so", "libroctx64.so"}) {
            if (void* h = dlopen(lib, RTLD_NOW | RTLD_GLOBAL)) {
                push = (int (*)(const char*))dlsym(h, "roctxRangePushA");
                pop = (int (*)())dlsym(h, "roctxRangePop");
                if (push && pop) return;
                push = nullptr;
                pop = nullptr;
            }
        }
    }
};
inline Roctx& roctx() {
    static Roctx r;
    return r;
}
// Consts::nt_cold by size: un-profiled bench.py pairs on one box (tools/nt_threshold.sh) — 2 M particles: +2 % with the hint, 4 M: +-1.5 %,
// 8 M: -1.8 %, 16 M: -1.3 % (profiles/r06_experiments/cold_stores.txt)
constexpr uint32_t NT_COLD_FROM = 6000000u;
// Consts::xcd_shift: chunks of 128 blocks of 256 particles (xcd_bid; a context of fewer than 8 x 128 blocks falls back to contiguous
// eighths by construction).  Measured at 16 M and 1 M, from t = 0 and in the late windows (profiles/r06_experiments/xcd_chunks.txt):
// 32 ... 128 blocks are within noise of each other, 512 costs 0.3-0.8 %, 2 048 gives half the late windows' gain back.
inline uint32_t xcd_shift_of(const sphx_ctx* c) { return c->xcd_chunk >= 0 ? xcd_shift_clamp(c->xcd_chunk) : 7u; }
// Launch wrapper: `bytes` = algorithmic HBM bytes of this launch (DESIGN.md §4), used for the roofline line of bench.py.
// sweeps = false: a launch that touches no particle in the expected case (the thin correction) leaves the direction alone, like the scan.
template <class F>
inline void launch(sphx_ctx* c, const char* name, double bytes, F&& f, bool sweeps = true) {
    Roctx& rx = roctx();
    if (rx.push) rx.push(name);
    struct Pop {
        Roctx& r;
        ~Pop() {
            if (r.pop) r.pop();
        }
    } pop_on_exit{rx};
    // (xcd_bid: every sweep over the particles starts where its predecessor stopped.  Not the scan — it runs over the cell table — and
    // not the scatter: between the density correction and the gather the scan and the scatter stream ~260 MB, a cache's worth; with the
    // scatter keeping the correction's direction the GATHER turns round against both: -0.4 % per step over toggling at every launch)
    if (sweeps && c->alternate_sweep && std::strcmp(name, "cell_scan") != 0 && !(c->alternate_sweep != 2 && std::strcmp(name, "cell_scatter") == 0)) c->K.rev ^= 1u;
    c->K.xcd_shift = xcd_shift_of(c);
    c->K.nt_cold = c->nt_cold_stores < 0 ? (c->N >= NT_COLD_FROM ? 1u : 0u) : (uint32_t)c->nt_cold_stores;
    if (c->profiling && (c->prof_filter.empty() || (c->prof_filter == name && (c->prof_counter++ % c->prof_every) == 0))) {
        ProfPending p{name, bytes, prof_event(c), prof_event(c)};
        hipEventRecord(p.a, c->stream);
        f();
        hipEventRecord(p.b, c->stream);
        c->prof_pending.push_back(p);
        if (c->prof_pending.size() > 4096) prof_resolve(c);
    } else {
        f();
    }
    // debugging aid (SPHX_TRACE_LAUNCH=1): every launch is named on stderr and waited for — a device fault names its kernel
    static const bool trace = [] { const char* e = std::getenv("SPHX_TRACE_LAUNCH"); return e && e[0] == '1'; }();
    if (trace) {
        std::fprintf(stderr, "[sphx] %s ...", name);
        const hipError_t e = hipStreamSynchronize(c->stream);
        std::fprintf(stderr, " %s\n", e == hipSuccess ? "ok" : hipGetErrorString(e));
    }
}

// ---- memory ------------------------------------------------------------------------------------------------------
template <class T>
int dev_alloc(sphx_ctx* c, T** p, size_t count) {
    if (*p) {
        hipFree(*p);
        *p = nullptr;
    }
    if (count == 0) count = 1;
    // (+GAT2_PAD: the staging's two-slots-per-lane loads may read one record past the last slot of an array, gat2 / nb_stage_load)
    SPHX_HIP(c, hipMalloc((void**)p, count * sizeof(T) + GAT2_PAD));
    return SPHX_OK;
}
template <class T>
void dev_free(T** p) {
    if (*p) hipFree(*p);
    *p = nullptr;
}

// device temporaries of the inspection calls: freed on every return path
template <class T>
struct DevTemp {
    T* p = nullptr;
    ~DevTemp() {
        if (p) hipFree(p);
    }
    hipError_t alloc(size_t count) { return hipMalloc((void**)&p, std::max<size_t>(count, 1) * sizeof(T) + GAT2_PAD); }  // (pad: as dev_alloc)
    operator T*() const { return p; }
};

void free_grid(Grid& g) {
    dev_free(&g.dir);
    dev_free(&g.dirn);
    dev_free(&g.fine);
    dev_free(&g.hist);
    dev_free(&g.tile_empty);
    g = Grid();
}

// host restatement of cell_of (same IEEE ops as the device): used to size the block directories only
inline uint32_t host_sat_u16(float v) {
    if (!(v > 0.0f)) return 0;
    if (v >= 65535.0f) return 65535;
    return (uint32_t)v;
}
inline uint32_t host_part1by1(uint32_t x) {
    x &= 0xffffu;
    x = (x ^ (x << 8)) & 0x00ff00ffu;
    x = (x ^ (x << 4)) & 0x0f0f0f0fu;
    x = (x ^ (x << 2)) & 0x33333333u;
    x = (x ^ (x << 1)) & 0x55555555u;
    return x;
}
inline uint32_t host_morton(uint32_t x, uint32_t y) { return (host_part1by1(y) << 1) | host_part1by1(x); }
inline void host_cell(const sphx_ctx* c, const float* xy, uint32_t& cx, uint32_t& cy) {
    cx = host_sat_u16((xy[0] - c->K.gmin_x) * c->K.cell_inv);
    cy = host_sat_u16((xy[1] - c->K.gmin_y) * c->K.cell_inv);
}

bool cell_bbox(const sphx_ctx* c, const float* xy, uint32_t n, uint32_t out[4]) {
    if (n == 0) return false;
    uint32_t x0 = 0xFFFFFFFFu, y0 = 0xFFFFFFFFu, x1 = 0, y1 = 0;
    for (uint32_t i = 0; i < n; ++i) {
        uint32_t cx, cy;
        host_cell(c, xy + 2 * (size_t)i, cx, cy);
        x0 = std::min(x0, cx);
        y0 = std::min(y0, cy);
        x1 = std::max(x1, cx);
        y1 = std::max(y1, cy);
    }
    out[0] = x0;
    out[1] = y0;
    out[2] = x1;
    out[3] = y1;
    return true;
}

// DIR_STATIC of a dynamic directory entry: does the boundary's directory cover block (bx, by)?  The neighbour build skips its whole
// static section for wavefronts whose 3x3 boxes touch no such block.
inline bool static_covers(const sphx_ctx* c, uint32_t bx, uint32_t by) {
    const Grid& s = c->gstat;
    if (bx - s.bx0 >= s.nbx || by - s.by0 >= s.nby || s.cover.empty()) return false;
    return s.cover[(size_t)(by - s.by0) * s.nbx + (bx - s.bx0)] != 0;
}
// The neighbour build's directory (NbGrid, sphx_internal.hpp) from the host copy of the plain one: uncovered blocks -> the null block
// behind the cell table, flags stripped, DIRN_FLAG set as described there.  g.dirn holds max(nbx * nby, 1) entries.
int upload_dirn(sphx_ctx* c, Grid& g) {
    const bool dyn = &g == &c->gdyn;
    const uint32_t null_off = g.len();
    std::vector<uint32_t> dn(std::max<size_t>(g.h_dir.size(), 1), null_off | (dyn ? DIRN_FLAG : 0u));
    for (uint32_t y = 0; y < g.nby; ++y)
        for (uint32_t x = 0; x < g.nbx; ++x) {
            const uint32_t e = g.h_dir[(size_t)y * g.nbx + x];
            if (e == EMPTY) continue;
            bool flag = !dyn;
            for (int dy = -1; dy <= 1 && !flag; ++dy)
                for (int dx = -1; dx <= 1 && !flag; ++dx) flag = static_covers(c, g.bx0 + x + (uint32_t)dx, g.by0 + y + (uint32_t)dy);
            dn[(size_t)y * g.nbx + x] = (e & ~DIR_FLAGS) | (flag ? DIRN_FLAG : 0u);
        }
    SPHX_HIP(c, hipMemcpyAsync(g.dirn, dn.data(), dn.size() * 4, hipMemcpyHostToDevice, c->stream));
    SPHX_HIP(c, hipStreamSynchronize(c->stream));  // `dn` is a local vector
    return SPHX_OK;
}
int refresh_static_flags(sphx_ctx* c) {
    Grid& g = c->gdyn;
    if (g.h_dir.empty()) return SPHX_OK;
    int rcn = upload_dirn(c, g);
    if (rcn) return rcn;
    for (uint32_t y = 0; y < g.nby; ++y)
        for (uint32_t x = 0; x < g.nbx; ++x) {
            uint32_t& e = g.h_dir[(size_t)y * g.nbx + x];
            if (e != EMPTY) e = (e & ~DIR_STATIC) | (static_covers(c, g.bx0 + x, g.by0 + y) ? DIR_STATIC : 0u);
        }
    SPHX_HIP(c, hipMemcpyAsync(g.dir, g.h_dir.data(), g.h_dir.size() * 4, hipMemcpyHostToDevice, c->stream));
    SPHX_HIP(c, hipStreamSynchronize(c->stream));
    return SPHX_OK;
}

// Build the block directory of a grid on the host and upload it: the blocks of the rectangle [bx0,bx1]x[by0,by1] (all of
// them, or only those flagged in `occ`) are numbered in ascending Morton order of (bx,by), which makes the fine table's
// layout the global Morton order of cells.  (Re)allocates the fine/hist tables; hist is left all-zero.
int set_directory(sphx_ctx* c, Grid& g, uint32_t bx0, uint32_t by0, uint32_t bx1, uint32_t by1, const std::vector<uint8_t>* occ, bool empty) {
    SPHX_HIP(c, hipStreamSynchronize(c->stream));
    const uint32_t nbx = empty ? 0 : bx1 - bx0 + 1, nby = empty ? 0 : by1 - by0 + 1;
    std::vector<std::pair<uint32_t, uint32_t>> blocks;
    for (uint32_t y = 0; y < nby; ++y)
        for (uint32_t x = 0; x < nbx; ++x) {
            const uint32_t lin = y * nbx + x;
            if (!occ || (*occ)[lin]) blocks.push_back({host_morton(bx0 + x, by0 + y), lin});
        }
    std::sort(blocks.begin(), blocks.end());
    if ((uint64_t)blocks.size() * BLOCK_CELLS > 0x7FFFFFFFull) return c->fail(SPHX_ERR_CAPACITY, "cell table larger than 2^32 entries");
    std::vector<uint32_t> dir((size_t)nbx * nby, EMPTY);
    for (size_t r = 0; r < blocks.size(); ++r)
        dir[blocks[r].second] = (uint32_t)(r * BLOCK_CELLS) | ((occ && (*occ)[blocks[r].second] == 2) ? DIR_FRINGE : 0u);
    if (&g == &c->gdyn)
        for (uint32_t y = 0; y < nby; ++y)
            for (uint32_t x = 0; x < nbx; ++x)
                if (dir[(size_t)y * nbx + x] != EMPTY && static_covers(c, bx0 + x, by0 + y)) dir[(size_t)y * nbx + x] |= DIR_STATIC;
    int rc;
    if (dir.size() > g.dir_cap || !g.dir || !g.dirn) {  // never null: the kernels load entry 0 unconditionally
        if ((rc = dev_alloc(c, &g.dir, dir.size())) || (rc = dev_alloc(c, &g.dirn, dir.size()))) return rc;
        SPHX_HIP(c, hipMemsetAsync(g.dir, 0xFF, std::max<size_t>(dir.size(), 1) * 4, c->stream));
        g.dir_cap = (uint32_t)dir.size();
    }
    // Everything below goes onto the context's stream: a plain hipMemset / hipMemcpy runs on the null stream, which a non-blocking
    // stream does not wait for — a histogram memset could then land in the middle of the next build (seen as a handful of particles
    // losing their cell once in ~15 runs of the random-cloud tile test).
    if (!dir.empty()) {
        SPHX_HIP(c, hipMemcpyAsync(g.dir, dir.data(), dir.size() * 4, hipMemcpyHostToDevice, c->stream));
        SPHX_HIP(c, hipStreamSynchronize(c->stream));  // `dir` is a local vector
    }
    g.bx0 = bx0;
    g.by0 = by0;
    g.nbx = nbx;
    g.nby = nby;
    g.nblk = (uint32_t)blocks.size();
    g.h_dir.swap(dir);
    g.fine_valid = false;
    const uint32_t len = g.len();
    if (len > g.fine_cap || !g.fine) {  // (the cell table is followed by the null block: NbGrid)
        if ((rc = dev_alloc(c, &g.fine, (size_t)len + BLOCK_CELLS)) || (rc = dev_alloc(c, &g.hist, std::max(len, 1u)))) return rc;
        g.fine_cap = len;
    }
    if (len) SPHX_HIP(c, hipMemsetAsync(g.hist, 0, (size_t)len * 4, c->stream));
    SPHX_HIP(c, hipMemsetAsync(g.fine, 0, ((size_t)len + BLOCK_CELLS) * 8, c->stream));
    if ((rc = upload_dirn(c, g))) return rc;
    const uint32_t ntile = nblocks(len, std::min(SCAN_TILE, SCAN1_TILE)) + 1;
    if (ntile > g.tile_cap || !g.tile_empty) {
        if ((rc = dev_alloc(c, &g.tile_empty, ntile))) return rc;
        g.tile_cap = ntile;
    }
    SPHX_HIP(c, hipMemsetAsync(g.tile_empty, 0x01, (size_t)g.tile_cap * 4, c->stream));  // the zeroed table says "empty" everywhere
    if (&g == &c->gdyn) c->pending.forget();  // a count made with the old directory is gone with the old histogram
    const uint32_t need = nblocks(len, std::min(SCAN_TILE, SCAN1_TILE)) + 1;
    if (need > c->scan_partials_cap) {
        if ((rc = dev_alloc(c, &c->scan_partials, need))) return rc;
        c->scan_partials_cap = need;
    }
    if (need > c->scan_state_cap) {
        if ((rc = dev_alloc(c, &c->scan_state, need))) return rc;
        SPHX_HIP(c, hipMemsetAsync(c->scan_state, 0, (size_t)need * 8, c->stream));
        c->scan_state_cap = need;
    }
    return SPHX_OK;
}

// Dynamic grid: SPARSE coverage.  Covered = the 64x64-cell blocks that hold particles plus a one-block FRINGE around them; blocks
// between far-apart pools are not in the table at all (two pools a kilometre apart cost two pools' worth of table, not a
// kilometre's).  A particle moves < 1 cell per step (CFL); k_key_count raises DF_NEAR_EDGE as soon as one lands in a fringe block,
// and the host then turns every fringe block into an interior one and puts a new fringe around them — 64 steps before a particle
// could reach uncovered ground.  Every covered block costs 4096 table entries in the per-step histogram scan, hence one ring.
// `cover` holds 0 (uncovered) / 1 (interior) / 2 (fringe) over the directory rectangle.
int apply_cover(sphx_ctx* c, uint32_t bx0, uint32_t by0, uint32_t bx1, uint32_t by1, std::vector<uint8_t>& cover) {
    Grid& g = c->gdyn;
    const uint32_t nbx = bx1 - bx0 + 1, nby = by1 - by0 + 1;
    // fringe: uncovered 8-neighbours of interior blocks (the rectangle was sized with room for them)
    for (uint32_t y = 0; y < nby; ++y)
        for (uint32_t x = 0; x < nbx; ++x) {
            if (cover[(size_t)y * nbx + x] != 1) continue;
            for (int dy = -1; dy <= 1; ++dy)
                for (int dx = -1; dx <= 1; ++dx) {
                    const int xx = (int)x + dx, yy = (int)y + dy;
                    if (xx < 0 || yy < 0 || xx >= (int)nbx || yy >= (int)nby) continue;
                    uint8_t& v = cover[(size_t)yy * nbx + xx];
                    if (v == 0) v = 2;
                }
        }
    int rc = set_directory(c, g, bx0, by0, bx1, by1, &cover, false);
    if (rc) return rc;
    g.cover.swap(cover);
    return SPHX_OK;
}

// positions (xy != nullptr): mark their blocks interior, merged with the present coverage.  grow: fringe -> interior, new fringe.
int cover_dynamic(sphx_ctx* c, const float* xy, uint32_t n, bool grow) {
    Grid& g = c->gdyn;
    const uint32_t MB = 65535u >> BLOCK_SHIFT;
    // blocks to add, as a bounding box first
    uint32_t ax0 = 0xFFFFFFFFu, ay0 = 0xFFFFFFFFu, ax1 = 0, ay1 = 0;
    std::vector<uint32_t> blocks;  // packed (by << 16) | bx of the particles' blocks (with repeats squeezed out by runs)
    if (xy) {
        uint32_t last = 0xFFFFFFFFu;
        for (uint32_t i = 0; i < n; ++i) {
            if (!std::isfinite(xy[2 * (size_t)i]) || !std::isfinite(xy[2 * (size_t)i + 1])) continue;
            uint32_t cx, cy;
            host_cell(c, xy + 2 * (size_t)i, cx, cy);
            const uint32_t bx = cx >> BLOCK_SHIFT, by = cy >> BLOCK_SHIFT, key = (by << 16) | bx;
            if (key == last) continue;
            last = key;
            blocks.push_back(key);
            ax0 = std::min(ax0, bx);
            ay0 = std::min(ay0, by);
            ax1 = std::max(ax1, bx);
            ay1 = std::max(ay1, by);
        }
    }
    if (blocks.empty() && !(grow && g.nbx)) return SPHX_OK;
    // new rectangle: old one and the additions, each with a ring of room for the fringe
    uint32_t bx0 = ax0, by0 = ay0, bx1 = ax1, by1 = ay1;
    if (g.nbx) {
        bx0 = std::min(bx0, g.bx0);
        by0 = std::min(by0, g.by0);
        bx1 = blocks.empty() ? g.bx0 + g.nbx - 1 : std::max(bx1, g.bx0 + g.nbx - 1);
        by1 = blocks.empty() ? g.by0 + g.nby - 1 : std::max(by1, g.by0 + g.nby - 1);
    }
    bx0 = bx0 > 0 ? bx0 - 1 : 0;
    by0 = by0 > 0 ? by0 - 1 : 0;
    bx1 = std::min(bx1 + 1, MB);
    by1 = std::min(by1 + 1, MB);
    const uint32_t nbx = bx1 - bx0 + 1, nby = by1 - by0 + 1;
    if ((uint64_t)nbx * nby > (1ull << 28)) return c->fail(SPHX_ERR_CAPACITY, "block directory larger than 2^28 entries");
    std::vector<uint8_t> cover((size_t)nbx * nby, 0);
    bool changed = g.cover.empty() || nbx != g.nbx || nby != g.nby || bx0 != g.bx0 || by0 != g.by0;
    for (uint32_t y = 0; y < g.nby && !g.cover.empty(); ++y)
        for (uint32_t x = 0; x < g.nbx; ++x) {
            uint8_t v = g.cover[(size_t)y * g.nbx + x];
            if (grow && v == 2) {
                v = 1;
                changed = true;
            }
            if (v) cover[(size_t)(g.by0 + y - by0) * nbx + (g.bx0 + x - bx0)] = v;
        }
    for (uint32_t key : blocks) {
        uint8_t& v = cover[(size_t)((key >> 16) - by0) * nbx + ((key & 0xFFFFu) - bx0)];
        if (v != 1) {
            v = 1;
            changed = true;
        }
    }
    if (!changed) return SPHX_OK;
    return apply_cover(c, bx0, by0, bx1, by1, cover);
}

// The coverage re-derived from what the cell table of the latest build holds: interior = the blocks with particles in them, fringe
// = one ring around those.  cover_dynamic(grow) only ever adds rings (a whole rim per particle that reaches the fringe, which keeps
// such events >= 64 steps apart); every COVER_PERIOD builds this takes the coverage back to what the fluid occupies: blocks it has
// left — splashes, a column that has collapsed — drop out of the table again, and with them their 4096 entries each in every
// build's histogram scan (the dam break at 1 M particles had grown from 8 to 31 us of scan after 3 750 steps).  One small kernel,
// one byte per block back to the host, one stream synchronisation per COVER_PERIOD steps.
constexpr uint32_t COVER_PERIOD = 256;
int cover_from_occupancy(sphx_ctx* c) {
    Grid& g = c->gdyn;
    c->builds_since_cover = 0;
    if (!g.nblk || !g.fine_valid || g.h_dir.size() != (size_t)g.nbx * g.nby) return SPHX_OK;
    DevTemp<uint8_t> occ_dev;
    SPHX_HIP(c, occ_dev.alloc(g.nblk));
    std::vector<uint8_t> occ(g.nblk);
    hipLaunchKernelGGL(k_block_occupancy, dim3(nblocks(g.nblk)), dim3(256), 0, c->stream, (const uint2*)g.fine, g.nblk, occ_dev.p);
    SPHX_HIP(c, hipMemcpyAsync(occ.data(), occ_dev.p, g.nblk, hipMemcpyDeviceToHost, c->stream));
    SPHX_HIP(c, hipStreamSynchronize(c->stream));
    const uint32_t MB = 65535u >> BLOCK_SHIFT;
    uint32_t ax0 = 0xFFFFFFFFu, ay0 = 0xFFFFFFFFu, ax1 = 0, ay1 = 0;
    std::vector<uint32_t> keep;  // (by << 16) | bx of the occupied blocks
    for (uint32_t y = 0; y < g.nby; ++y)
        for (uint32_t x = 0; x < g.nbx; ++x) {
            const uint32_t e = g.h_dir[(size_t)y * g.nbx + x];
            if (e == EMPTY || !occ[(e & ~DIR_FLAGS) / BLOCK_CELLS]) continue;
            const uint32_t bx = g.bx0 + x, by = g.by0 + y;
            keep.push_back((by << 16) | bx);
            ax0 = std::min(ax0, bx);
            ay0 = std::min(ay0, by);
            ax1 = std::max(ax1, bx);
            ay1 = std::max(ay1, by);
        }
    if (keep.empty()) return SPHX_OK;  // (no particle has a cell: nothing to go by — leave the coverage alone)
    const uint32_t bx0 = ax0 > 0 ? ax0 - 1 : 0, by0 = ay0 > 0 ? ay0 - 1 : 0, bx1 = std::min(ax1 + 1, MB), by1 = std::min(ay1 + 1, MB);
    const uint32_t nbx = bx1 - bx0 + 1, nby = by1 - by0 + 1;
    std::vector<uint8_t> cover((size_t)nbx * nby, 0);
    for (uint32_t key : keep) cover[(size_t)((key >> 16) - by0) * nbx + ((key & 0xFFFFu) - bx0)] = 1;
    // unchanged?  (compare the interior sets: the fringe follows from them)
    if (nbx == g.nbx && nby == g.nby && bx0 == g.bx0 && by0 == g.by0) {
        bool same = true;
        for (size_t k = 0; k < cover.size() && same; ++k) same = (cover[k] == 1) == (g.cover[k] == 1);
        if (same) return SPHX_OK;
    }
    return apply_cover(c, bx0, by0, bx1, by1, cover);
}

// Static grid: exact block occupancy of the boundary particles (thin lines -> few blocks), computed on the host.
int cover_static(sphx_ctx* c) {
    const uint32_t n = c->B;
    if (n == 0) {
        c->gstat.cover.clear();
        int rc0 = set_directory(c, c->gstat, 0, 0, 0, 0, nullptr, true);
        return rc0 ? rc0 : refresh_static_flags(c);
    }
    uint32_t box[4];
    cell_bbox(c, c->h_boundary.data(), n, box);
    const uint32_t bx0 = box[0] >> BLOCK_SHIFT, by0 = box[1] >> BLOCK_SHIFT, bx1 = box[2] >> BLOCK_SHIFT, by1 = box[3] >> BLOCK_SHIFT;
    const uint32_t nbx = bx1 - bx0 + 1, nby = by1 - by0 + 1;
    std::vector<uint8_t> occ((size_t)nbx * nby, 0);
    for (uint32_t i = 0; i < n; ++i) {
        uint32_t cx, cy;
        host_cell(c, c->h_boundary.data() + 2 * (size_t)i, cx, cy);
        occ[(size_t)((cy >> BLOCK_SHIFT) - by0) * nbx + ((cx >> BLOCK_SHIFT) - bx0)] = 1;
    }
    int rc = set_directory(c, c->gstat, bx0, by0, bx1, by1, &occ, false);
    if (rc) return rc;
    c->gstat.cover.swap(occ);
    return refresh_static_flags(c);  // the dynamic directory's DIR_STATIC bits follow the boundary
}

// ---- host <- device scalars ---------------------------------------------------------------------------------------------
// The publishing kernel writes the mailbox fields, a system-scope fence, then `seq`.  The host spins briefly on the pinned
// word and falls back to a stream synchronise, so correctness never depends on how promptly the write becomes visible.
int wait_mailbox(sphx_ctx* c, uint32_t seq) {
    volatile uint32_t* p = &c->mbox->seq;
    bool got = false;
    // "reached", not "equals": with sphx_step_begin_law later publishers are already queued behind the one waited for
    auto reached = [&] { return (int32_t)(*p - seq) >= 0; };
    for (int spin = 0; spin < 200000; ++spin) {
        if (reached()) {
            got = true;
            break;
        }
        __builtin_ia32_pause();
    }
    if (!got) {
        SPHX_HIP(c, hipStreamSynchronize(c->stream));
        if (!reached()) return c->fail(SPHX_ERR_HIP, "device did not publish the step scalars (kernel fault?)");
    }
    __atomic_thread_fence(__ATOMIC_ACQUIRE);
    const unsigned long long cum = c->mbox->nb_entries;
    if (cum != c->nb_cum) {
        c->nb_last = cum - c->nb_cum;
        c->nb_cum = cum;
    }
    const unsigned long long rm = c->mbox->rem_entries;
    if (rm != c->rem_cum) {
        c->rem_last = rm - c->rem_cum;
        c->rem_cum = rm;
    }
    const unsigned long long ow = c->mbox->owned_cum;
    if (ow != c->owned_cum) {
        c->owned_last = ow - c->owned_cum;
        c->owned_cum = ow;
    }
    const uint32_t f = c->mbox->flags;
    if (f) hipLaunchKernelGGL(k_clear_flags, dim3(1), dim3(1), 0, c->stream, c->d_scal, f);  // exactly the bits seen here
    if (f & DF_NB_CAP) c->step_flags |= SPHX_FLAG_NEIGHBOR_CAP;
    if (f & DF_HALO_CAP) return c->fail(SPHX_ERR_CAPACITY, "halo exchange buffer too small for the particles near a tile cut");
    if (f & DF_NEAR_EDGE) c->need_expand = true;
    if (f & DF_STRAY) {
        c->step_flags |= SPHX_FLAG_STRAY_PARTICLES;
        c->need_recover = true;
    }
    if (f & DF_DENSE_CELL) c->step_flags |= SPHX_FLAG_DENSE_CELL;
    if (f & DF_SCAN_STALL) return c->fail(SPHX_ERR_HIP, "the cell-table scan stalled waiting for a predecessor workgroup");
    if (f & DF_NONFINITE) return c->fail(SPHX_ERR_NONFINITE, "a solver residual is not finite (dfsph.rs:223 / :378 assert)");
    if (f & DF_OUT_OF_DOMAIN) return c->fail(SPHX_ERR_OUT_OF_DOMAIN, "a particle left the Morton domain the grid tables were sized for, or has no cell at all (a NaN position)");
    if (f & DF_NB_PANIC) return c->fail(SPHX_ERR_NEIGHBOR_PANIC, "64 dynamic neighbours and a static hit (neighborhood_search.rs:373 panics here)");
    return SPHX_OK;
}

int publish_and_wait(sphx_ctx* c) {
    const uint32_t seq = ++c->seq;
    hipLaunchKernelGGL(k_publish, dim3(1), dim3(64), 0, c->stream, c->d_scal, c->mbox_dev, seq);
    return wait_mailbox(c, seq);
}

// The density correction of a step may have left the NEXT build's cell count in gdyn.hist / key (CountArgs).  Whoever
// needs those buffers clean, or changes what the count was made with, calls this first.
void wipe_histogram(sphx_ctx* c, Grid& g) {
    if (g.hist && g.len()) hipMemsetAsync(g.hist, 0, (size_t)g.len() * 4, c->stream);
}
void drop_fused_count(sphx_ctx* c) {
    if (c->pending.drop()) wipe_histogram(c, c->gdyn);
}
// A call that failed on the device (SPHX_ERR_HIP, SPHX_ERR_NONFINITE) may have stopped between a cell count and the scatter that
// counts the histogram back down: with or without a pending fused count, neither histogram is known to be zero any more.  Called by
// step_finish's failure path and by every sphx_upload (new positions: any count made before is void anyway), so that a failure in
// any entry point — step_begin's warm-up build included — is cleaned up by the re-upload the context then asks for.
void clear_histograms(sphx_ctx* c) {
    c->pending.forget();
    for (Grid* g : {&c->gdyn, &c->gstat}) wipe_histogram(c, *g);
}

// A cell count made by a tile's density correction (TileClassArgs) is made from ADVECTED positions and leaves out what the tile
// retires: it is only good for the packing pass that takes over from there (tile_pack_impl).  Whoever else comes first drops it.
void drop_class_count(sphx_ctx* c) {
    if (c->pending.drop_if_from_classifier()) wipe_histogram(c, c->gdyn);
}
// tile path: see sphx_ctx::tile_pending_dt
void flush_pending_advect(sphx_ctx* c) {
    // (entry points call this before their own hipSetDevice; the launches and the memset below must target THIS context's device —
    // in-process multi-device tiles run each tile on a host thread whose current device is still 0)
    if (c->pending.from_classifier() || c->tile_pending_dt > 0.0f) (void)hipSetDevice(c->device);
    drop_class_count(c);
    if (!(c->tile_pending_dt > 0.0f)) return;
    const uint32_t n = c->tile_pending_n;
    const float dt = c->tile_pending_dt;
    c->tile_pending_dt = 0.0f;
    c->tile_pending_n = 0;
    const bool fix = c->tile_fix_owner;
    c->tile_fix_owner = false;
    if (!n) return;
    if (fix) {
        // the step's classification was made by its last density correction (TileClassArgs) and the records are out: what the gather
        // was going to do on the way — advection, owner bits of the new ghosts — and the marks of the retired particles, by the full
        // packing kernel with nobody to send to
        TilePeers none{};
        hipLaunchKernelGGL(k_tile_pack, dim3(nblocks(n)), dim3(256), 0, c->stream, (const float2*)c->vel, c->posA, c->pid, (const float*)c->kappa,
                           (const float*)c->stiff, n, c->K, c->tile_halo, none, (const uint32_t*)c->tile_blk, 0u, dt, CountArgs{}, c->d_scal, 1u,
                           (const uint32_t*)nullptr);
        return;
    }
    hipLaunchKernelGGL(k_advect, dim3(nblocks(n)), dim3(256), 0, c->stream, c->posA, (const float2*)c->vel, n, dt);
}

// What every sub-step entry point that reads or moves the particles starts with: a pass that ran ahead is stale from here, and what
// the packing pass left to the re-grid's gather is done on the spot (with it goes a classifier's count nobody took over).
void sub_step_enter(sphx_ctx* c) {
    c->ahead.valid = false;
    flush_pending_advect(c);
}

// ---- grid build (a1-a4) -------------------------------------------------------------------------------------------
// Sorts `n` points into Morton cell order (stable) and leaves the cell table in g.fine.  Attribute arrays in `ga` are
// gathered alongside; the caller swaps its buffers afterwards.  advect_dt > 0: the fluid build inside a step — the position
// update x += v* dt is fused into the first kernel.  5 launches.
// tile_n != nullptr (multi-GPU tile re-grid): `n` is an upper bound that includes dropped (NaN) slots; the number of particles
// that actually received a cell is published to the mailbox under the sequence number returned through *tile_n.
int build_grid(sphx_ctx* c, Grid& g, const float2* pos, uint32_t n, const GatherArgs& ga, float advect_dt, bool ring, uint32_t* tile_n = nullptr,
               bool mark_velocities = false) {
    hipStream_t st = c->stream;
    DevScalars* ds = c->d_scal;
    const uint32_t len = g.len();
    const uint32_t nt = nblocks(len, c->scan_two_pass ? SCAN_TILE : SCAN1_TILE);
    const bool counted = &g == &c->gdyn && advect_dt > 0 && !tile_n && c->pending.is_for(n);
    // tile path: the packing pass or sphx_tile_count_kept has counted the first so many particles while the halo exchange was in flight
    const bool partial = &g == &c->gdyn && tile_n && advect_dt == 0.0f && !counted && c->pending.is_for_first_of(n);
    const uint32_t first = partial ? c->pending.n() : 0u;
    if (&g == &c->gdyn) c->velmarks.wrote();  // (the gather below moves every velocity: an earlier gather's marks describe the old array)
    if (&g == &c->gdyn) c->accel_uniform.velocities_written();
    if (counted || partial)
        c->pending.forget();  // consumed: k_scatter counts the histogram back down to zero, as behind any count (the scan leaves it as it is)
    else
        drop_fused_count(c);  // (the other grid's build too: key is shared)
    if (n > first && !counted) {
        const uint32_t gbc = std::max(1u, nblocks(n - first));
        if (advect_dt > 0)
            launch(c, "advect+cell_count", (16.0 + 4 + 4) * n, [&] {
                hipLaunchKernelGGL(k_key_count<true>, dim3(gbc), dim3(256), 0, st, c->pv(), (const float2*)nullptr, n, advect_dt, c->K,
                                   g.view(), g.hist, c->key, ring ? 1u : 0u, ds, first);
            });
        else
            launch(c, "cell_count", (8.0 + 4 + 4) * (n - first), [&] {
                hipLaunchKernelGGL(k_key_count<false>, dim3(gbc), dim3(256), 0, st, PVr{nullptr, nullptr}, pos, n, 0.0f, c->K, g.view(),
                                   g.hist, c->key, ring ? 1u : 0u, ds, first);
            });
    }
    // no table at all (a tile that owns nothing yet): the count of sorted particles is zero — it must not keep the value another
    // build (the static grid shares the scalar) left there
    if (!len) hipMemsetAsync(&ds->sort_total, 0, 4, st);
    uint32_t scan_seq = 0;
    if (len)
        launch(c, "cell_scan", (c->scan_two_pass ? 20.0 : 16.0) * len, [&] {
            if (c->scan_two_pass) {
                hipLaunchKernelGGL(k_scan_reduce, dim3(nt), dim3(256), 0, st, (const uint32_t*)g.hist, len, c->scan_partials, ds, &ds->sort_total);
                hipLaunchKernelGGL(k_scan_apply, dim3(nt), dim3(256), 0, st, g.hist, g.fine, len, (const uint32_t*)c->scan_partials);
                hipMemsetAsync(g.tile_empty, 0, (size_t)g.tile_cap * 4, st);  // (this form rewrites every range: nothing is known to be empty-and-unwritten)
            } else {
                if (++c->scan_epoch == 0) c->scan_epoch = 1;  // 0 is what a fresh state array holds
                if (tile_n) scan_seq = ++c->seq;  // tile path: the scan's last workgroup publishes the new local count itself
                hipLaunchKernelGGL(k_scan_onepass, dim3(nt), dim3(256), 0, st, g.hist, g.fine, len, c->scan_state, c->scan_epoch, ds, &ds->sort_total,
                                   tile_n ? c->mbox_dev : (Mailbox*)nullptr, scan_seq, g.tile_empty, tile_n ? 0xFFFFFFFFu : n);
            }
        });
    g.fine_valid = len != 0;
    if (n) {
        launch(c, "cell_scatter", 12.0 * n, [&] {
            hipLaunchKernelGGL(k_scatter, dim3((nblocks(n, 256 * SCATTER_PER_LANE) + 7u) & ~7u), dim3(256), 0, st, (const uint32_t*)c->key, n, (const uint2*)g.fine,
                               c->order, g.hist, xcd_scatter_pack(c->K.rev, xcd_shift_of(c)));  // (its blocks hold 1 024 particles)
        });
        const uint32_t ng = n;
        if (tile_n) {
            // the count of particles that received a cell stays on the device: the gather (and the neighbour build after it) run over
            // the upper bound and clip themselves; the host picks the number up from the mailbox once those are queued
            if (scan_seq) {
                *tile_n = scan_seq;
            } else {
                const uint32_t seq = ++c->seq;
                hipLaunchKernelGGL(k_publish, dim3(1), dim3(64), 0, st, ds, c->mbox_dev, seq);
                *tile_n = seq;
            }
        }
        const uint32_t gb2 = std::max(8u, (nblocks(ng, 256 * GATHER_PER_LANE) + 7u) & ~7u);
        double gbytes = 4;  // order (cell index and cell range only where a cell reaches out of the window of order[] words)
        gbytes += ga.vel_in ? (16 + 16) : 16;
        if (ga.r_in) gbytes += 8;
        if (ga.r2_in) gbytes += 8;
        if (ga.r3_in) gbytes += 8;
        if (ga.u_in) gbytes += 8;
        // rigid motion (mark_velocities: update_neighborhood's decision): the gather says which velocities differ from vel_in[0] (VelMarks)
        GatherArgs gm = ga;
        if (mark_velocities && &g == &c->gdyn && !tile_n && ga.vel_in) {
            if (++c->gather_seq == 0) c->gather_seq = 1;  // 0 is what fresh mark words hold
            gm.vmix_tag = c->gather_seq;
        }
        if (ng)
            launch(c, "gather_attributes", gbytes * ng, [&] {
                hipLaunchKernelGGL(k_rank_gather, dim3(gb2), dim3(256), 0, st, (const uint32_t*)c->order, (const uint32_t*)c->key, ng, n,
                                   (const uint2*)g.fine, gm, tile_n ? (const uint32_t*)&ds->sort_total : (const uint32_t*)nullptr, xcd_pack(c->K.rev, xcd_shift_of(c)));
            });
        if (ng && gm.vmix_tag) c->velmarks.made(gm.vmix_tag);
    }
    return SPHX_OK;
}

int ensure_index_scratch(sphx_ctx* c) {
    // key/slot/order are shared by the dynamic and the static grid build: size them for the larger of the two
    const uint32_t need = std::max(std::max(std::max(c->N, c->capN), c->B), 1u);
    if (need <= c->idx_cap) return SPHX_OK;
    int rc;
    if ((rc = dev_alloc(c, &c->key, need))) return rc;
    if ((rc = dev_alloc(c, &c->order, need))) return rc;
    SPHX_HIP(c, hipMemsetAsync(c->order, 0, (size_t)need * 4, c->stream));
    c->idx_cap = need;
    return SPHX_OK;
}

// Field sampling (sphx_sample_*, sphx_sample.inc) reads the cell grids and density[]: a query is refused (SPHX_ERR_NOT_READY, with
// `missing` as the message) from here until a neighbour build AND the densities of its positions have completed (sphx_ctx::sample_ready).
static inline void sample_went_stale(sphx_ctx* c, const char* missing) {
    c->sample_ready = 0u;
    c->tile_density_ready = false;
    c->sample_missing = missing;
}
// A finished step whose neighbour build ran (sample_ready == 1: the build completed, its densities are the step's) may be sampled.  A
// step over zero fluid particles runs no build: the static grid of a new boundary may not exist yet.
static inline void sample_after_step(sphx_ctx* c) {
    if (c->sample_ready == 1u)
        c->sample_ready = 2u;
    else
        sample_went_stale(c, "no neighbour build has run since the particles or the boundary changed (a step over zero fluid particles runs "
                             "none): call sphx_update_neighborhood + sphx_update_densities");
}
// The recorder of sphx_track_record (sphx_track.inc): a finished step tests one flag; with a recording on, a frame of the tracked set is
// queued behind the step's kernels.
void track_take_frame(sphx_ctx* c);
static inline void track_after_step(sphx_ctx* c) {
    if (c->track.recording) track_take_frame(c);
}
// The recorder of sphx_stats_record (sphx_stats.inc), likewise: one flag test; with a recording on, a frame of statistics is queued
// behind the step's kernels.
void stats_take_frame(sphx_ctx* c, float dt);
static inline void stats_after_step(sphx_ctx* c, float dt) {
    if (c->stats.recording) stats_take_frame(c, dt);
}
// The recorder of sphx_probe_record (sphx_gauge.inc), likewise: one flag test; with a recording on, a frame of point probes and gauge
// records is queued behind the step's kernels (only where the finished step left a state that may be sampled).
void probe_take_frame(sphx_ctx* c, float dt);
static inline void probe_after_step(sphx_ctx* c, float dt) {
    if (c->probe.recording) probe_take_frame(c, dt);
}
// Positions are about to change (or have changed) without the neighbour lists being rebuilt first: the walks go back to the forms
// that are right for any distance (sqrt_dist in sphx_kernels.hip) until the next build.
static inline void lists_went_stale(sphx_ctx* c) {
    c->K.q_noclamp = 0u;
    c->lists_current = false;
    c->quiet_hint[0] = c->quiet_hint[1] = false;  // (another scene, for all the corrections know)
    c->rigid_forget();
    if (c->d_scal) hipMemsetAsync(&c->d_scal->spec.flags, 0, sizeof(uint32_t), c->stream);  // (... and no speculative flag of the old one)
    // (a caller that has already dropped the sampling state keeps its own, more specific message)
    if (c->sample_ready) sample_went_stale(c, "the positions changed since the last neighbour build: run a step, or sphx_update_neighborhood + sphx_update_densities");
}

// (Re)allocate the [N|B] arrays for capN fluid + capB boundary slots, keeping the fluid prefix of posA/vel — and, while the tail does
// not move (capN unchanged: sphx_set_boundary with a larger boundary), the boundary tail the current lists still point into: the
// previous boundary stays in place until the next re-grid (DESIGN.md section 5, "Deliberate difference"), the half step before it walks the old lists over it.
int ensure_nb_arrays(sphx_ctx* c, uint32_t needN, uint32_t needB, bool keep_fluid) {
    const uint32_t newN = std::max(c->capN, needN), newB = std::max(c->capB, std::max(needB, 1u));
    if (newN == c->capN && newB == c->capB && c->vel) return SPHX_OK;
    const size_t tot = (size_t)newN + newB;
    // the kernels gather 16-byte records with 32-bit byte offsets (gat()): 2^28 slots = 268 M particles per context
    if (tot >= ((size_t)1 << 28)) return c->fail(SPHX_ERR_CAPACITY, "more than 2^28 fluid + boundary slots in one context: split the domain into tiles");
    float2* old_pos = c->posA;
    float2* old_vel = c->vel;
    c->posA = nullptr;
    c->vel = nullptr;
    int rc;
    // (+ 4 slots behind the positions: the neighbour build re-reads out-of-window candidates four at a time, whatever the run's length)
    if ((rc = dev_alloc(c, &c->posA, tot + 4)) || (rc = dev_alloc(c, &c->posA2, tot + 4)) || (rc = dev_alloc(c, &c->vel, tot)) ||
        (rc = dev_alloc(c, &c->vel2, tot)))
        return rc;
    if (keep_fluid && c->N && old_vel) {
        SPHX_HIP(c, hipMemcpyAsync(c->posA, old_pos, (size_t)c->N * 8, hipMemcpyDeviceToDevice, c->stream));
        SPHX_HIP(c, hipMemcpyAsync(c->vel, old_vel, (size_t)c->N * 8, hipMemcpyDeviceToDevice, c->stream));
        SPHX_HIP(c, hipStreamSynchronize(c->stream));
    }
    if (keep_fluid && old_vel && newN == c->capN && c->B && !c->tails_dirty) {
        // (the new tail beyond the old boundary's records: zeros — no list points there yet)
        const size_t off = (size_t)c->capN, nb = std::min<size_t>(c->B, c->capB);
        SPHX_HIP(c, hipMemsetAsync(c->posA + off, 0, ((size_t)newB + 4) * 8, c->stream));
        SPHX_HIP(c, hipMemsetAsync(c->vel + off, 0, (size_t)newB * 8, c->stream));
        SPHX_HIP(c, hipMemcpyAsync(c->posA + off, old_pos + off, nb * 8, hipMemcpyDeviceToDevice, c->stream));
        // (the OTHER pair of arrays too: the first density iteration predicts into vel2 and swaps — its boundary tail must read v = 0,
        // and a gather target's tail the same positions, whichever array is current when the half step runs)
        SPHX_HIP(c, hipMemsetAsync(c->posA2 + off, 0, ((size_t)newB + 4) * 8, c->stream));
        SPHX_HIP(c, hipMemsetAsync(c->vel2 + off, 0, (size_t)newB * 8, c->stream));
        SPHX_HIP(c, hipMemcpyAsync(c->posA2 + off, old_pos + off, nb * 8, hipMemcpyDeviceToDevice, c->stream));
        SPHX_HIP(c, hipStreamSynchronize(c->stream));
    }
    dev_free(&old_pos);
    dev_free(&old_vel);
    c->tails_dirty = true;  // the boundary tail moved (soff = capN) or does not exist yet
    // the FAST walks (sqrt_dist<true>, no clamp of q) assume lists built from the records they read: not across a reallocation
    lists_went_stale(c);
    // capN / capB are committed by the callers (alloc_particles / sphx_set_boundary)
    return SPHX_OK;
}

// NeighborhoodSearch::update_static (neighborhood_search.rs:488-491)
int build_static(sphx_ctx* c) {
    int rc;
    if ((rc = cover_static(c))) return rc;
    GatherArgs ga{};
    ga.flags = c->d_scal;
    ga.pos_in = c->bpos;
    ga.pos_out = c->bpos2;
    ga.u_in = c->bid;
    ga.u_out = c->bid2;
    if ((rc = build_grid(c, c->gstat, c->bpos, c->B, ga, 0.0f, false))) return rc;
    std::swap(c->bpos, c->bpos2);
    std::swap(c->bid, c->bid2);
    c->boundary_changed = false;
    c->tails_dirty = true;
    return SPHX_OK;
}

int fill_tails(sphx_ctx* c) {
    if (c->B)
        hipLaunchKernelGGL(k_fill_tails, dim3(nblocks(c->B)), dim3(256), 0, c->stream, (const float2*)c->bpos, c->B, c->soff(), c->posA, c->posA2,
                           c->vel, c->vel2);
    c->tails_dirty = false;
    return SPHX_OK;
}

// A particle outran the covered rectangle (DF_STRAY; rare: a blow-up or a huge fixed step).  Fetch the records, take the bounding
// box of where the particles will be after this build's advection, and cover it — unless that box is absurd (a particle on its
// way to infinity): then the strays stay clamped, neighbour-less, and the next attempt waits 64 builds.
int recover_directory(sphx_ctx* c, float advect_dt, uint32_t advect_below = 0xFFFFFFFFu) {
    const uint32_t n = c->N;
    if (!n) return SPHX_OK;
    std::vector<float> hp((size_t)n * 2), hv((size_t)n * 2);
    SPHX_HIP(c, hipMemcpyAsync(hp.data(), c->posA, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
    SPHX_HIP(c, hipMemcpyAsync(hv.data(), c->vel, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
    SPHX_HIP(c, hipStreamSynchronize(c->stream));
    std::vector<float> xy((size_t)n * 2);
    size_t m = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const float dt_i = i < advect_below ? advect_dt : 0.0f;  // (records behind a deferred tile advection are already where they will be)
        const float x = hp[2 * (size_t)i] + hv[2 * (size_t)i] * dt_i, y = hp[2 * (size_t)i + 1] + hv[2 * (size_t)i + 1] * dt_i;
        if (std::isfinite(x) && std::isfinite(y)) {
            xy[2 * m] = x;
            xy[2 * m + 1] = y;
            m += 1;
        }
    }
    if (!m) return SPHX_OK;
    // how many blocks would that cover?  (distinct blocks x 9 bounds blocks + fringe)
    std::vector<uint32_t> keys;
    keys.reserve(m);
    for (size_t i = 0; i < m; ++i) {
        uint32_t cx, cy;
        host_cell(c, xy.data() + 2 * i, cx, cy);
        keys.push_back(((cy >> BLOCK_SHIFT) << 16) | (cx >> BLOCK_SHIFT));
    }
    std::sort(keys.begin(), keys.end());
    const size_t distinct = (size_t)(std::unique(keys.begin(), keys.end()) - keys.begin());
    if ((uint64_t)distinct * 9 * BLOCK_CELLS > (1ull << 26)) {  // > 64 M table entries (0.75 GiB of tables): not a fluid any more
        c->recover_cooldown = 64;
        return SPHX_OK;
    }
    return cover_dynamic(c, xy.data(), (uint32_t)m, false);
}

// The per-wavefront "some k is not +-0" words for the producers of kbuf (k_compute_error, k_neighbor_build<2>): single context only,
// nullptr with SPHX_ZERO_SKIP=0, and by default in a context of fewer than 4 M particles.
inline uint32_t* zero_skip_flags(const sphx_ctx* c) { return c->zero_skip_on() && !c->tile_mode ? c->knz : nullptr; }

// FluidParticleWorld::update_neighborhood_datastructure (fluidparticleworld.rs:235-261).
// extra_alpha: also permute alpha_values (warm-up, dfsph.rs:425).  Velocities (vel[] — the predicted velocities inside a
// step, dfsph.rs:512) and ids always follow.  advect_dt > 0: fuse the advection (dfsph.rs:499-510) into the re-grid.
// fuse: compute density + alpha inside the neighbour build (dfsph.rs:516-518).
// fuse_div: the build also does the first compute_density_change of the divergence loop that follows (dfsph.rs:521 -> :249-280):
// same neighbours, same order, and the positions and kernel gradients are already in registers — one full list traversal less per
// step.  Only when that loop starts without a warm start (the warm start changes the velocities first).
// fuse_warm: the other case — the divergence loop starts WITH a warm start (dfsph.rs:354-360): that traversal (it needs positions,
// gradients and the slot-bound warm-start values, all known here, and changes only the particle's own velocity) rides on the build.
int update_neighborhood(sphx_ctx* c, bool extra_alpha, float advect_dt, bool fuse, bool fuse_div = false, bool fuse_warm = false) {
    int rc;
    drop_class_count(c);
    c->lists_current = false;
    sample_went_stale(c, "the last neighbour build did not complete: upload the state again");
    if (c->boundary_changed) {
        if ((rc = build_static(c))) return rc;
    }
    if (c->tails_dirty) fill_tails(c);
    if (c->need_expand) {
        c->need_expand = false;
        if ((rc = cover_dynamic(c, nullptr, 0, true))) return rc;
    } else if (++c->builds_since_cover >= COVER_PERIOD) {
        if ((rc = cover_from_occupancy(c))) return rc;
    }
    // the positions the directory has to cover are the ADVECTED ones: inside a step advect_dt says so; on the tile path the packing
    // pass may have left the advection of the first tile_pending_n records to this re-grid's gather (tile_pending_dt) — covering the
    // blocks of the positions as they still are would let fast movers land outside the freshly covered ground (round-3 advisor finding)
    const float cover_dt = advect_dt > 0.0f ? advect_dt : (c->tile_pending_dt > 0.0f ? c->tile_pending_dt : 0.0f);
    const uint32_t cover_below = advect_dt > 0.0f ? 0xFFFFFFFFu : c->tile_pending_n;
    if (c->tile_mode && c->gdyn.nblk == 0 && c->N) {
        // a tile that owned nothing has received its first records: give them cells before this build (an empty table cannot even
        // park them)
        if ((rc = recover_directory(c, cover_dt, cover_below))) return rc;
    }
    if (c->need_recover) {  // strays seen: re-cover before this build and, predictively, before the next few (fast movers keep moving)
        c->need_recover = false;
        c->recover_streak = 8;
    }
    if (c->recover_streak) {
        c->recover_streak -= 1;
        if (c->recover_cooldown) {
            c->recover_cooldown -= 1;
        } else if ((rc = recover_directory(c, cover_dt, cover_below))) {
            return rc;
        }
    }
    GatherArgs ga{};
    ga.flags = c->d_scal;
    ga.pos_in = c->posA;
    ga.pos_out = c->posA2;
    ga.vel_in = c->vel;
    ga.vel_out = c->vel2;
    ga.advect_dt = advect_dt;  // the advection of dfsph.rs:499-510 is applied by the gather (the key pass only looks at the new position)
    ga.advect_below = 0xFFFFFFFFu;
    if (extra_alpha) {
        ga.r_in = c->alpha;
        ga.r_out = c->alpha2;
    }
    ga.u_in = c->pid;
    ga.u_out = c->pid2;
    uint32_t tile_n = c->N;
    // (a single context in tiling-invariant mode moves the warm-start values like a tile does)
    const bool carry_kappa = c->tile_mode ? c->tile_carry_kappa : c->tiling_invariant, carry_stiff = c->tile_mode ? c->tile_carry_stiff : c->tiling_invariant;
    ga.rank_by_id = c->tiling_invariant ? 1u : 0u;
    ga.nt_cold = c->nt_cold_stores < 0 ? (c->N >= NT_COLD_FROM ? 1u : 0u) : (uint32_t)c->nt_cold_stores;
    // (a warm-start array whose values the next solver loop will zero before it reads them need not travel: sphx_tile_carry_warmstart)
    if (carry_kappa) {
        ga.r2_in = c->kappa;
        ga.r2_out = c->kappa2;
    }
    if (carry_stiff) {
        ga.r3_in = c->stiff;
        ga.r3_out = c->stiff2;
    }
    if (c->tile_mode) ga.count_owned = c->d_scal;
    if (c->tile_pending_dt > 0.0f) {
        // the packing pass left the advection of the kept particles to this gather — which is only right if its cell count (made
        // from the advected positions) is still the one this build starts from
        if (c->tile_mode && advect_dt == 0.0f && c->pending.is_for(c->tile_pending_n) && c->tile_pending_n <= c->N) {
            ga.advect_dt = c->tile_pending_dt;
            ga.advect_below = c->tile_pending_n;
            c->tile_pending_dt = 0.0f;
            c->tile_pending_n = 0;
            if (c->tile_fix_owner) {
                c->tile_fix_owner = false;
                ga.fix_owner = 1u;
                ga.cell_inv = c->K.cell_inv;
                ga.gmin_x = c->K.gmin_x;
                ga.gmin_y = c->K.gmin_y;
                ga.own = c->K.tile;
            }
        } else {
            flush_pending_advect(c);
        }
    }
    // Take-over of the divergence loop (below): the fused build stores the warm-start sums and the loop's first correction is thin.
    // Decided here, once, because the gather's marks (rigid motion) are worth writing exactly where that correction follows: no warm
    // start in front of the loop, nothing but a thin correction between the gather and the run-ahead pass.  A disturbed scene has no
    // quiet hint, so its gather writes no mark (250 k wavefronts storing into 32 lines: +5 ... +9 us per step at 16 M, 2500 steps in,
    // profiles/rigid_skip/ab_16M_1M.txt).
    const bool take_div = fuse && fuse_div && !fuse_warm && zero_skip_flags(c) && c->take_over(true);
    if ((rc = build_grid(c, c->gdyn, c->posA, c->N, ga, advect_dt, true, c->tile_mode ? &tile_n : nullptr, take_div && advect_dt > 0.0f && c->rigid_on())))
        return rc;
    if (carry_kappa) std::swap(c->kappa, c->kappa2);
    if (carry_stiff) std::swap(c->stiff, c->stiff2);
    std::swap(c->vel, c->vel2);
    std::swap(c->posA, c->posA2);
    if (extra_alpha) std::swap(c->alpha, c->alpha2);
    std::swap(c->pid, c->pid2);
    // NeighborLists::update (neighborhood_search.rs:399-423)
    c->K.q_noclamp = c->fast_walk_ok;  // from this build on the lists belong to the positions (sqrt_dist, sphx_kernels.hip)
    hipStream_t st = c->stream;
    const uint32_t* n_dev = c->tile_mode ? (const uint32_t*)&c->d_scal->sort_total : (const uint32_t*)nullptr;
    if (c->N) {
        const uint32_t n = c->N;
        auto go = [&](auto kernel, const DivArgs& dv) {
            hipLaunchKernelGGL(kernel, dim3(nblocks(n)), dim3(256), 0, st, (const float2*)c->posA, n, c->soff(), c->K, c->gdyn.nview(), c->gstat.nview(),
                               c->nb_list, c->nb_counts, c->nb_wave, c->nb_remote, c->density, c->alpha, c->d_scal, n_dev, dv);
        };
        c->handoff.clear();
        if (fuse && fuse_warm) {
            DivArgs dv{};
            dv.velw = c->vel;
            dv.warm = c->stiff;
            dv.lim = -0.5f * c->K.rho0 * c->K.rho0;
            launch(c, "neighbor_build+density_alpha+divergence_warmstart", (8.0 + list_bytes(c) + 8.0 + 8.0 + 8.0 + 4.0) * n, [&] { go(k_neighbor_build<3>, dv); });
            c->handoff = BuildHandoff::warm_applied();
            c->velmarks.wrote();  // (the warm start corrects velocities behind the gather)
            c->accel_uniform.velocities_written();
        } else if (fuse && fuse_div) {
            DivArgs dv{};
            dv.vel = (const float2*)c->vel;
            dv.kbuf = c->kbuf;
            dv.knz = zero_skip_flags(c);
            // the scene-wide mark goes under the number the divergence loop's first iteration will get when it is queued next
            // (sphx_step_finish does that; BuildHandoff::take_first_errors drops the flags if something took the number in between)
            dv.knz_tag = c->res_seq + 1u;
            // take-over: the loop's first correction stores 0 + k into the stiffness whatever path it takes, and nothing reads the
            // array between this build and that correction — under the quiet hint the build stores it, and the correction can be thin
            const bool take = take_div;
            if (take) {
                dv.warm = c->stiff;
                c->takeover_producers += 1;
            }
            launch(c, "neighbor_build+density_alpha+density_change", (8.0 + list_bytes(c) + 8.0 + 8.0 + 4.0) * n,
                   [&] { take ? go(k_neighbor_build<2, true>, dv) : go(k_neighbor_build<2>, dv); });
            c->handoff = BuildHandoff::first_errors(dv.knz != nullptr, dv.knz_tag, take);
        } else if (fuse)
            launch(c, "neighbor_build+density_alpha", (8.0 + list_bytes(c) + 8.0) * n, [&] { go(k_neighbor_build<1>, DivArgs{}); });
        else
            launch(c, "neighbor_build", (8.0 + list_bytes(c)) * n, [&] { go(k_neighbor_build<0>, DivArgs{}); });
    }
    if (c->tile_mode && c->N) {
        if ((rc = wait_mailbox(c, tile_n))) return rc;  // tile_n carries the sequence number of the publish inside build_grid
        c->N = std::min(c->mbox->sort_total, c->N);
    }
    c->lists_current = true;
    c->sample_ready = 1u;  // (the callers that also complete the densities of this build raise it to 2)
    c->sample_missing = "the densities of the last neighbour build are missing: call sphx_update_densities";
    return SPHX_OK;
}

template <int KIND>
void launch_density(sphx_ctx* c, bool density, bool alpha) {
    const uint32_t n = c->N;
    if (!n) return;
    const double bytes = (8.0 + list_bytes(c) + (density ? 4 : 0) + (alpha ? 4 : 0)) * n;
    auto go = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(nblocks(n)), dim3(256), 0, c->stream, (const float2*)c->posA, n, c->soff(), c->K, c->nbv(), c->density, c->alpha);
    };
    if (density && alpha) return launch(c, "density_alpha", bytes, [&] { go(k_density_alpha<KIND, true, true>); });
    if (density) return launch(c, "update_densities", bytes, [&] { go(k_density_alpha<KIND, true, false>); });
    launch(c, "compute_alpha_factors", bytes, [&] { go(k_density_alpha<0, false, true>); });
}

// What every reader of accel[] starts with (sphx::AccelUniform, DESIGN.md §4): a rigid non-pressure pass may have left the array
// unwritten, and the fill it left out goes in front of the reader (k_accel_materialize decides on the device whether there is
// anything to fill).  read_accel: a copy that leaves the velocities alone.  take_accel: the first consumer, a velocity prediction —
// substitute: the density producer's rigid form, which reads K.a from its arguments while nothing has written a velocity since the pass.
void fill_accel(sphx_ctx* c, const AccelUniform::Taken& t) {
    const uint32_t n = std::min(c->N, c->capN);
    if (!t.fill || !n || !c->accel) return;
    const uint32_t vgrid = nblocks(n);
    launch(c, "accel_materialize", 8.0 * n, [&] {
        hipLaunchKernelGGL(k_accel_materialize, dim3(std::min(vgrid, 2048u)), dim3(256), 0, c->stream, c->accel, n, vgrid, c->K.ax, c->K.ay,
                           (const DevScalars*)c->d_scal, t.tag);
    }, false);
}
void read_accel(sphx_ctx* c) { fill_accel(c, c->accel_uniform.read()); }
AccelUniform::Taken take_accel(sphx_ctx* c, bool substitute) {
    const AccelUniform::Taken t = c->accel_uniform.take(substitute);
    fill_accel(c, t);
    return t;
}

// cap: the capacity to allocate when n does not fit (0: exactly n).  keep_set (sphx_append): positions, velocities and ids of [0, N)
// survive the reallocation too.
int alloc_particles(sphx_ctx* c, uint32_t n, uint32_t cap = 0, bool keep_set = false) {
    if (n <= c->capN) return SPHX_OK;
    cap = std::max(cap, n);
    int rc = 0;
    if ((rc = ensure_nb_arrays(c, cap, c->capB, keep_set))) return rc;
    // keep the slot-wise warm-start values of the reference's Vec::resize (dfsph.rs:420-422)
    float *old_kappa = c->kappa, *old_stiff = c->stiff, *old_alpha = c->alpha;
    float2* old_accel = c->accel;  // WCSPH: `accellerations` is slot-bound too (Vec::resize, wscsph.rs:129)
    uint32_t* old_pid = keep_set ? c->pid : nullptr;
    if (keep_set) c->pid = nullptr;
    const uint32_t keep = std::min(c->cached_n, c->capN);
    const uint32_t keep_accel = std::min(c->wcsph_n, c->capN);
    // (a rigid pass may owe the old array its fill: paid where the array is copied, forgotten with the array otherwise)
    keep_accel ? read_accel(c) : c->accel_uniform.filled();
    c->kappa = c->stiff = c->alpha = nullptr;
    c->accel = nullptr;
    auto give_up = [&](int code) {  // an allocation failed: the old slot-bound arrays are of no use without their siblings
        dev_free(&old_kappa);
        dev_free(&old_stiff);
        dev_free(&old_alpha);
        dev_free(&old_accel);
        dev_free(&old_pid);
        c->cached_n = 0;
        c->wcsph_n = 0;
        c->uploaded = false;
        return code;
    };
#define A(p) \
    if ((rc = dev_alloc(c, &c->p, cap))) return give_up(rc);
    A(accel) A(density) A(alpha) A(alpha2) A(kappa) A(stiff) A(kappa2) A(stiff2) A(pid) A(pid2) A(nb_counts) A(kbuf)
#undef A
    if ((rc = dev_alloc(c, &c->knz, (size_t)(nblocks(cap) + 8) * 4))) return give_up(rc);  // (one word per wavefront of the rounded-up grid, like nb_wave)
    if ((rc = dev_alloc(c, &c->nb_remote, (size_t)(nblocks(cap) + 8) * REMOTE_CAP))) return give_up(rc);
    if ((rc = dev_alloc(c, &c->nb_wave, (size_t)(nblocks(cap) + 8) * 4))) return give_up(rc);
    const size_t slices = ((size_t)cap + 63) / 64;
    if ((rc = dev_alloc(c, &c->nb_list, slices * 64 * 64))) return give_up(rc);
    SPHX_HIP(c, hipMemsetAsync(c->kappa, 0, (size_t)cap * 4, c->stream));
    SPHX_HIP(c, hipMemsetAsync(c->stiff, 0, (size_t)cap * 4, c->stream));
    SPHX_HIP(c, hipMemsetAsync(c->alpha, 0, (size_t)cap * 4, c->stream));
    SPHX_HIP(c, hipMemsetAsync(c->density, 0, (size_t)cap * 4, c->stream));
    if (keep) {
        SPHX_HIP(c, hipMemcpyAsync(c->kappa, old_kappa, (size_t)keep * 4, hipMemcpyDeviceToDevice, c->stream));
        SPHX_HIP(c, hipMemcpyAsync(c->stiff, old_stiff, (size_t)keep * 4, hipMemcpyDeviceToDevice, c->stream));
        SPHX_HIP(c, hipMemcpyAsync(c->alpha, old_alpha, (size_t)keep * 4, hipMemcpyDeviceToDevice, c->stream));
    }
    if (keep_accel) SPHX_HIP(c, hipMemcpyAsync(c->accel, old_accel, (size_t)keep_accel * 8, hipMemcpyDeviceToDevice, c->stream));
    if (old_pid && c->N) SPHX_HIP(c, hipMemcpyAsync(c->pid, old_pid, (size_t)c->N * 4, hipMemcpyDeviceToDevice, c->stream));
    SPHX_HIP(c, hipStreamSynchronize(c->stream));
    dev_free(&old_kappa);
    dev_free(&old_stiff);
    dev_free(&old_alpha);
    dev_free(&old_accel);
    dev_free(&old_pid);
    c->capN = cap;
    return SPHX_OK;
}

// The device judges the residual itself (LoopArgs) unless the residual needs an all-reduce over tiles or the A/B switch is set.
inline bool device_loop(const sphx_ctx* c) { return !c->tile_mode && !c->host_loop; }

// ---- one solver iteration: a launcher per kernel family and the one path that queues them (DESIGN.md §4) ----------------------------
// Each launcher owns grid and block, the argument list, the choice of instantiation, the launch() label and the byte formula.

// v* = v + a dt (dfsph.rs:484-492).  va / tl: the kernel reads the non-pressure pass's maximum and derives dt itself (sphx_step_begin_law).
void launch_predict(sphx_ctx* c, const char* label, float dt, const VmaxArgs& va = VmaxArgs{}, const TimerLaw& tl = TimerLaw{}) {
    const uint32_t n = c->N;
    c->velmarks.wrote();
    take_accel(c, false);  // (k_predict reads accel[]: a fill the rigid pass left out comes first)
    launch(c, label, 24.0 * n, [&] { hipLaunchKernelGGL(k_predict, dim3(nblocks(n)), dim3(256), 0, c->stream, c->vel, (const float2*)c->accel, n, dt, c->d_scal, va, tl); });
}

// compute_density_error / compute_density_change (dfsph.rs:217 / :372).  pred != nullptr: the density kernel does the velocity
// prediction on the way, from accel[] into vel2[].  clear_hist: the cell count the previous iteration's correction left, wiped on the
// way.  (No warm_zero array: the zeroing of dfsph.rs:206-208 / :361-363 is implicit, the first correction starts the sum from zero.)
void launch_compute_error(sphx_ctx* c, bool divergence, float dt, const float* dt_dev, const LoopArgs& la, uint32_t* clear_hist, uint32_t clear_len,
                          const PredArgs* pred, uint32_t* knz, uint32_t knz_tag, bool take_warm = false,
                          const CountArgs& take_count = CountArgs{}) {
    const uint32_t n = c->N;
    const double lb = list_bytes(c);
    if (pred) c->velmarks.wrote();  // (the prediction folded in: vel2[] becomes the velocities)
    // warm: where a take-over producer stores the warm-start sums 0 + k; take: NoTake{}, or the speculative cell count that goes out with them
    auto go = [&](auto kernel, float* warm, const PredArgs& pa, auto take) {
        hipLaunchKernelGGL(kernel, dim3(nblocks(n)), dim3(256), 0, c->stream, c->pv(), (const float*)c->density, (const float*)c->alpha, n, c->soff(), c->K, dt,
                           c->nbv(), c->kbuf, warm, c->d_scal, dt_dev, la, clear_hist, clear_len, pa, knz, knz_tag, take);
    };
    if (divergence) {
        launch(c, "compute_density_change", (16 + 4 + 4 + lb) * n, [&] {
            if (knz && take_warm) return go(k_compute_error<true, false, true, true>, c->stiff, PredArgs{}, NoTake{});  // (take-over: the sums 0 + k go out with k)
            if (knz) return go(k_compute_error<true, false, true>, nullptr, PredArgs{}, NoTake{});
            go(k_compute_error<true>, nullptr, PredArgs{}, NoTake{});
        });
    } else if (pred) {
        PredArgs pa = *pred;
        pa.accel = c->accel;
        pa.vel_out = c->vel2;
        // Rigid motion: the first consumer of accel[] behind a rigid non-pressure pass.  As the take-over producer, with every grad W
        // finite, it takes the record for itself and reads K.a from its arguments (k_compute_error_rigid); any other form reads the
        // array, behind the fill the pass left out.
        const AccelUniform::Taken au = take_accel(c, c->rigid_predict != 0 && knz && take_warm && c->K.q_noclamp && !c->tile_mode);
        if (au.k_a) {
            c->rigid_predict_launches += 1;
            const RigidTake rt{take_count, au.tag, c->zero_skip_count ? 1u : 0u};
            auto go_rigid = [&](auto kernel) {
                hipLaunchKernelGGL(kernel, dim3(nblocks(n)), dim3(256), 0, c->stream, c->pv(), (const float*)c->density, (const float*)c->alpha, n, c->soff(), c->K, dt,
                                   c->nbv(), c->kbuf, c->kappa, c->d_scal, dt_dev, la, clear_hist, clear_len, pa, knz, knz_tag, rt);
            };
            // (the exit's stream: own position, density, alpha, count word; k, v*, kappa, the cell word and its count)
            const double bytes = c->rigid_predict == 2 ? (8 + 4 + 4 + 2 + 4 + 8 + 4 + 4 + 8) * (double)n : (16 + 8 + 4 + 4 + 4 + lb) * n;
            return launch(c, "velocity_prediction+compute_density_error", bytes,
                          [&] { c->rigid_predict == 2 ? go_rigid(k_compute_error_rigid<true>) : go_rigid(k_compute_error_rigid<false>); });
        }
        launch(c, "velocity_prediction+compute_density_error", (16 + 8 + 8 + 4 + 4 + 4 + lb) * n, [&] {
            if (knz && take_warm) return go(k_compute_error<false, true, true, true>, c->kappa, pa, take_count);  // (take-over: kappa = 0 + k and the count go out too)
            if (knz) return go(k_compute_error<false, true, true>, nullptr, pa, NoTake{});
            go(k_compute_error<false, true>, nullptr, pa, NoTake{});
        });
    } else {
        launch(c, "compute_density_error", (16 + 4 + 4 + 4 + lb) * n + (clear_hist ? 4.0 * clear_len : 0.0), [&] {
            if (knz && take_warm) return go(k_compute_error<false, false, true, true>, c->kappa, PredArgs{}, take_count);
            if (knz) return go(k_compute_error<false, false, true>, nullptr, PredArgs{}, NoTake{});
            go(k_compute_error<false>, nullptr, PredArgs{}, NoTake{});
        });
    }
}

// correct_velocity_with_{density,divergence}_error (dfsph.rs:218 / :373).  ca.hist: the density correction also makes the next build's
// cell count (+8 B per particle); tc.pid: and the tile's send classification (+4 B).
// knz: the flags this iteration's producer wrote (nullptr: none) — handed to the kernel only where a skipped walk is an exact identity.
// (q_noclamp: the lists were built from these positions, every grad W is finite; a dt the device derives is tested by the kernel)
inline bool correct_skip_ok(const sphx_ctx* c, bool divergence, float dt, const float* dt_dev, const TileClassArgs& tc, const uint32_t* knz) {
    const float inv_dt = 1.0f / dt;
    return knz && c->K.q_noclamp && !tc.pid && std::isfinite(c->K.mass) && c->K.mass > 0.0f && (dt_dev || divergence || (inv_dt > 0.0f && std::isfinite(inv_dt)));
}
void launch_correct(sphx_ctx* c, bool divergence, float dt, const float* dt_dev, const CountArgs& ca, const LoopArgs& la, const ResArgs& ra, bool first,
                    const TileClassArgs& tc, const uint32_t* knz, bool warm_taken = false) {
    const uint32_t n = c->N, f = first ? 1u : 0u;
    const float inv_dt = 1.0f / dt, lim = -0.5f * c->K.rho0 * c->K.rho0;
    const char* const label = divergence ? "correct_velocity_with_divergence_error" : "correct_velocity_with_density_error";
    float* warm = divergence ? c->stiff : c->kappa;
    const bool skip_ok = correct_skip_ok(c, divergence, dt, dt_dev, tc, knz);
    const ZeroSkipArgs zs{skip_ok ? knz : nullptr, c->zero_skip_count ? 1u : 0u};
    // The decide-first form (quiet scene) only while this loop's latest correction saw no mark: a workgroup that walks pays a round
    // trip for looking first.  A hint — either form computes the same bits whatever the scene is.
    const bool quiet_first = zs.knz && c->quiet_hint[divergence ? 1 : 0];
    // The thin form (take-over): a first correction whose producer has stored the warm-start sums.  2 048 workgroups (k_correct's
    // resident generation, 8 per CU x 256 CUs) stand for the whole grid; a quiet scene costs them one look at the marks.  256 ... 4 096
    // measure alike, 16 384 is slower (profiles/quiet_takeover/ab_16M_1M.txt).
    // (density loop: the producer has also made the cell count, speculatively — enqueue_iteration takes over only where this launch
    // will be thin, so that every speculative count meets the kernel that confirms or corrects it)
    const bool thin = first && warm_taken && zs.knz && (divergence || ca.hist);
    if ((quiet_first || thin) && c->zero_skip_count) c->qf_launches += 1;
    // (rigid motion: a thin correction writes velocities only with its iteration's mark set, which the consumer reads; any other form voids)
    thin ? c->velmarks.thin(ra.rseq) : c->velmarks.wrote();
    c->accel_uniform.velocities_written();
    if (thin) {
        c->thin_launches += 1;
        const uint32_t vblocks = nblocks(n);
        auto go_thin = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, dim3(std::min(vblocks, c->thin_grid ? c->thin_grid : 2048u)), dim3(256), 0, c->stream, c->vel, (const float2*)c->posA,
                               (const float*)c->kbuf, warm, n, c->soff(), c->K, inv_dt, lim, c->nbv(), dt_dev, ca, c->d_scal, la, ra, zs, vblocks);
        };
        const double bytes = (16 + 8 + 12 + 8 + list_bytes(c) + (ca.hist ? 8 : 0)) * n;
        return launch(c, label, bytes, [&] { divergence ? go_thin(k_correct_thin<false>) : go_thin(k_correct_thin<true>); }, false);
    }
    auto go = [&](auto kernel, const ZeroSkipArgs& zsa) {
        hipLaunchKernelGGL(kernel, dim3(nblocks(n)), dim3(256), 0, c->stream, c->vel, (const float2*)c->posA, (const float*)c->kbuf, warm, n, c->soff(), c->K, inv_dt,
                           lim, c->nbv(), dt_dev, ca, c->d_scal, la, ra, f, tc, zsa);
    };
    launch(c, label, (16 + 8 + 12 + 8 + list_bytes(c) + (ca.hist ? (tc.pid ? 8 + 4 : 8) : 0)) * n, [&] {
        // (a launch without flags runs the instantiation without the skip's decision: the code from before it)
        if (divergence && quiet_first) return go(k_correct<false, false, false, true, true>, zs);
        if (quiet_first) return go(k_correct<false, true, false, true, true>, zs);
        if (divergence && zs.knz) return go(k_correct<false, false, false, true>, zs);
        if (divergence) return go(k_correct<false, false>, zs);
        if (tc.pid) return go(k_correct<false, true, true>, ZeroSkipArgs{});
        if (zs.knz) return go(k_correct<false, true, false, true>, zs);
        go(k_correct<false, true>, zs);
    });
}

// The warm start in front of a loop (dfsph.rs:199-205 / :354-360).  labelled = false (the tile sub-step): a bare launch, outside
// launch() — no label, no profile record, and K.rev / K.xcd_shift / K.nt_cold stay as the launch before it left them.
void launch_warmstart(sphx_ctx* c, bool divergence, float dt, const float* dt_dev, bool labelled) {
    const uint32_t n = c->N;
    c->velmarks.wrote();
    c->accel_uniform.velocities_written();
    const float inv_dt = 1.0f / dt, lim = -0.5f * c->K.rho0 * c->K.rho0;
    auto one = [&](auto kernel, float* warm) {
        hipLaunchKernelGGL(kernel, dim3(nblocks(n)), dim3(256), 0, c->stream, c->vel, (const float2*)c->posA, (const float*)c->kbuf, warm, n, c->soff(), c->K, inv_dt,
                           lim, c->nbv(), dt_dev, CountArgs{}, c->d_scal, LoopArgs{}, ResArgs{}, 0u, TileClassArgs{}, ZeroSkipArgs{});
    };
    auto go = [&] { divergence ? one(k_correct<true, false>, c->stiff) : one(k_correct<true, true>, c->kappa); };
    if (!labelled) return go();
    // own position + velocity read, velocity written, staged positions, warm-start values
    launch(c, divergence ? "correct_divergence_error_warmstart" : "correct_density_error_warmstart", (16 + 8 + 8 + 4 + list_bytes(c)) * n, go);
}

// What one solver iteration is queued with: everything in which the single context's loops (enqueue_context_iteration) and the tile
// sub-steps (sub_iteration_impl) differ.  DESIGN.md §4 has the table.
struct IterSpec {
    bool divergence, first;          // first: first iteration of its loop (the correction starts the warm-start sum from zero)
    float dt;
    const float* dt_dev = nullptr;   // != nullptr: the kernels take the step from device memory
    uint32_t* out_warm = nullptr;    // != nullptr: the first iteration decides the warm start itself (dfsph.rs:199 / :354) and says so here
    const PredArgs* pred = nullptr;  // != nullptr: compute_density_error also does the velocity prediction — no k_predict in front
    LoopArgs la{};                   // enabled: the device judges the residual itself
    uint32_t* clear_hist = nullptr;  // handed to compute_density_error, with clear_len
    uint32_t clear_len = 0;
    CountArgs ca{};                  // hist != nullptr: the density correction counts the next build's cells ...
    bool drop_count = false;         // ... once the count an earlier correction left has been dropped
    TileClassArgs tc{};
};
inline CountArgs count_args(const sphx_ctx* c, float dt) { return CountArgs{c->gdyn.view(), c->gdyn.hist, c->key, dt}; }

// One iteration of a solver loop queued on the stream: [warm start, before the first one], compute_density_error /
// compute_density_change, correct_velocity_* (dfsph.rs:217-218 / :372-373).  The only place that does.  Returns the mailbox sequence
// number of the residual.
uint32_t enqueue_iteration(sphx_ctx* c, const IterSpec& s) {
    if (s.out_warm && s.first) {
        const bool warm = (s.divergence ? c->num_divergence_iters : c->num_density_iters) > 1;  // dfsph.rs:199 / :354
        *s.out_warm = warm ? 1u : 0u;
        if (warm && !(s.divergence && c->handoff.take_warm()))  // (taken: the neighbour build has applied it)
            launch_warmstart(c, s.divergence, s.dt, s.dt_dev, true);
    }
    const uint32_t seq = ++c->seq;
    const ResArgs ra{1u, ++c->res_seq, c->mbox_dev, seq};  // the correction reads (and publishes) the residual its compute_error leaves
    // the flags the correction may trust: the ones the producer of THIS iteration's kbuf wrote
    uint32_t* knz = s.tc.pid ? nullptr : zero_skip_flags(c);
    bool warm_taken = false;  // take-over: this iteration's producer has stored the warm-start sums its correction would store
    const BuildHandoff::Taken built = c->handoff.take_first_errors(s.divergence && s.first, ra.rseq);
    if (built.fused) {  // the neighbour build has left this iteration's errors, residual and zeroed warm-start values
        if (!built.flags_usable) knz = nullptr;
        warm_taken = knz && built.warm_taken;
    } else {
        // (a count an earlier correction left is dropped in FRONT of this compute_error: under the take-over it makes the new one)
        if (s.drop_count) drop_fused_count(c);
        // density loop: only with the count to make, and only where the correction will be thin (launch_correct's conditions)
        warm_taken = s.first && knz && c->take_over(s.divergence) && (s.divergence || (s.ca.hist && correct_skip_ok(c, false, s.dt, s.dt_dev, s.tc, knz)));
        if (warm_taken) c->takeover_producers += 1;
        launch_compute_error(c, s.divergence, s.dt, s.dt_dev, s.la, s.clear_hist, s.clear_len, s.pred, knz, ra.rseq, warm_taken, s.ca);
    }
    if (s.pred) std::swap(c->vel, c->vel2);  // the predicted velocities are the velocities from here on (the boundary tail is zero in both)
    if (s.drop_count) drop_fused_count(c);  // (the fused-build path; a no-op behind the one above)
    // the correction below counts (tc.pid: and classifies, with this dt)
    if (s.ca.hist) s.tc.pid ? c->pending.made_by_classifier(c->N, s.dt) : c->pending.made_by_correction(c->N);
    launch_correct(c, s.divergence, s.dt, s.dt_dev, s.ca, s.la, ra, s.first, s.tc, knz, warm_taken);
    return seq;
}

// The single context's form of it.  dt_dev: queued by sphx_step_begin_law before the host knows dt.  iter: 1-based index inside its
// loop; gen: generation number of a device-run loop (0: the host judges the residual).  count_ok (the density loops of
// sphx_step_finish / _begin_law): the correction may do the re-grid's cell count.  pred (first density iteration, no warm start in
// front of it): the caller has NOT launched k_predict.
uint32_t enqueue_context_iteration(sphx_ctx* c, bool divergence, float dt, const float* dt_dev, uint32_t iter, uint32_t gen, uint32_t* out_warm, bool count_ok,
                                   const PredArgs* pred = nullptr) {
    IterSpec s{divergence, iter == 1, dt, dt_dev, out_warm, pred};
    if (gen) {
        s.la.enabled = 1;
        s.la.iter = iter;
        s.la.fixed = divergence ? c->P.fixed_divergence_iterations : c->P.fixed_density_iterations;
        s.la.max_iters = divergence ? c->P.max_divergence_iterations : c->P.max_density_iterations;
        s.la.gen = gen;
        s.la.n_total = c->N;
        s.la.tol = divergence ? c->P.max_divergence_error : c->P.max_avg_density_error;
        s.la.rho0 = c->K.rho0;
        s.la.dt = dt;
    }
    if (!divergence) s.clear_len = c->gdyn.len();
    if (!divergence && count_ok && !c->no_fused_count && !c->tile_mode && c->gdyn.len()) {
        // Every correction counts.  Host-run loop: the count of a correction that turned out not to be the last is dropped in front of
        // the next one; device-run loop: an iteration that follows another has its compute_error wipe that one's count.
        s.ca = count_args(c, dt);
        s.drop_count = !gen || s.first;
        if (!s.drop_count && c->pending.live()) s.clear_hist = c->gdyn.hist;
    }
    return enqueue_iteration(c, s);
}

// dfsph.rs:221-236 / :376-391 for one published residual sum; sets the iteration-cap flag like the reference prints its warning
int judge_residual(sphx_ctx* c, bool divergence, double err_sum, uint32_t iters, float dt, float* out_avg, bool* out_more, uint32_t* io_flags) {
    const uint32_t n = c->N;
    const float rho0 = c->K.rho0;
    const uint32_t fixed = divergence ? c->P.fixed_divergence_iterations : c->P.fixed_density_iterations;
    const uint32_t max_iters = divergence ? c->P.max_divergence_iterations : c->P.max_density_iterations;
    const float tol = divergence ? c->P.max_divergence_error : c->P.max_avg_density_error;
    const float sum = (float)err_sum;  // exact fixed-point sum, rounded once (DESIGN.md §3)
    float avg;
    if (divergence) {
        avg = sum / (float)n / rho0;  // dfsph.rs:376-377
        if (!std::isfinite(avg)) return c->fail(SPHX_ERR_NONFINITE, "avg_divergence is not finite (dfsph.rs:378)");
    } else {
        avg = sum / (float)n;  // dfsph.rs:221
        if (!std::isfinite(avg)) return c->fail(SPHX_ERR_NONFINITE, "avg_density_error is not finite (dfsph.rs:223)");
    }
    bool more;
    if (fixed) {
        more = iters < fixed;
    } else {
        const float rel = divergence ? avg : avg / rho0;  // dfsph.rs:222
        more = !(rel * dt < tol);                         // dfsph.rs:226 / :381
        if (more && iters > max_iters) {                  // dfsph.rs:236 / :391
            *io_flags |= divergence ? SPHX_FLAG_DIVERGENCE_ITER_CAP : SPHX_FLAG_DENSITY_ITER_CAP;
            more = false;
        }
    }
    *out_avg = avg;
    *out_more = more;
    return SPHX_OK;
}

// Wait until the device-run loop `gen` has terminated, or until iteration sequence `seq` has published without terminating it.
int wait_loop(sphx_ctx* c, uint32_t seq, uint32_t gen, bool* out_done) {
    volatile uint32_t* ps = &c->mbox->seq;
    volatile uint32_t* pg = &c->mbox->loop_gen_done;
    bool done = false, reached = false;
    for (int spin = 0; spin < 400000; ++spin) {
        if (*pg == gen) {
            done = true;
            break;
        }
        if ((int32_t)(*ps - seq) >= 0) {
            reached = true;
            break;
        }
        __builtin_ia32_pause();
    }
    if (!done && !reached) {
        SPHX_HIP(c, hipStreamSynchronize(c->stream));
        done = *pg == gen;
        if (!done && (int32_t)(*ps - seq) < 0) return c->fail(SPHX_ERR_HIP, "device did not publish the solver residual (kernel fault?)");
    }
    __atomic_thread_fence(__ATOMIC_ACQUIRE);
    if (!done) done = *pg == gen;  // the terminating iteration may be the one waited for
    *out_done = done;
    return SPHX_OK;
}

// Next slot of the vmax ring (Stripe::vmax: every reduction uses one, its reader clears the one that comes into use two reductions
// later).  A non-pressure pass that ran ahead and was discarded (sphx_ctx::ahead) has used a slot nobody read: that slot is cleared
// and handed out again, so the ring keeps its one-slot-per-reduction rhythm.
uint32_t take_vmax_slot(sphx_ctx* c) {
    if (c->ahead.queued) {
        c->ahead.queued = c->ahead.valid = false;
        hipLaunchKernelGGL(k_clear_vmax_slot, dim3(1), dim3(64), 0, c->stream, c->d_scal, c->ahead.vslot);
        return c->ahead.vslot;
    }
    return c->vmax_seq++ & 3u;
}

// The non-pressure pass of dfsph.rs:436-477 (accelerations + max |v + a dt_prev|^2 into vmax slot `vslot`).
// marks (the run-ahead launch only): what the latest fluid gather's marks say about vel[] (VelMarks).  With the record usable and the
// identity's conditions met the pass is judged: queued in the rigid form under the hint (k_nonpressure_rigid reports itself), else in
// today's form with k_rigid_judge behind it.  A launch that is not judged drops the hint.
inline bool finite_not_neg_zero(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return std::isfinite(f) && u != 0x80000000u;
}
// DESIGN.md §4, "Rigid motion": K.a + (+0) = K.a; every f finite (current lists, a normal rho0 dt, finite model constants)
inline bool rigid_conditions(const sphx_ctx* c, float dt) {
    const float rd = c->K.rho0 * dt;
    const float fc = c->VK.visc_model == SPHX_VISCOSITY_PHYSICAL ? c->VK.mu * c->K.mass * c->VK.vis_nlap * c->K.h : c->K.xsph_eps * c->K.mass * c->K.p6_norm;
    return c->rigid_on() && c->K.q_noclamp && c->lists_current && finite_not_neg_zero(c->K.ax) && finite_not_neg_zero(c->K.ay) && dt > 0.0f &&
           std::isfinite(dt) && std::isfinite(rd) && rd >= 1.175494351e-38f && std::isfinite(fc);
}
void enqueue_nonpressure(sphx_ctx* c, float dt_prev, uint32_t vslot, const VelMarks::Taken& marks = VelMarks::Taken{}) {
    const uint32_t n = c->N;
    const bool judged = marks.usable && rigid_conditions(c, dt_prev);
    // (fill: SPHX_RIGID_PREDICT=0 — the rigid form stores K.a itself, as it did before its consumer could read K.a from its arguments)
    const RigidArgs ra{marks.tag, marks.knz_tag, marks.check_knz ? 1u : 0u, nblocks(n), c->mbox_dev, c->rigid_predict == 0 ? 1u : 0u};
    c->rigid_judged = judged ? marks.tag : 0u;
    if (!judged) c->rigid_hint = false;
    if (judged && (c->rigid_skip == 2 || c->rigid_hint)) {
        c->rigid_launches += 1;
        ra.fill ? c->accel_uniform.filled() : c->accel_uniform.made(marks.tag);  // (what the pass owes accel[]: taken by its first reader)
        auto go_rigid = [&](auto kernel, auto visc) {
            hipLaunchKernelGGL(kernel, dim3(std::min(ra.vgrid, c->thin_grid ? c->thin_grid : 2048u)), dim3(256), 0, c->stream, c->pv(), (const float*)c->density, n,
                               c->soff(), c->K, dt_prev, c->nbv(), c->accel, c->d_scal, vslot, visc, ra);
        };
        // (sweeps = false: the fill ends where the build's sweep ended, which is where the kernel behind it starts)
        return launch(c, "nonpressure_accel_vmax", 8.0 * n, [&] {
            if (c->VK.visc_model == SPHX_VISCOSITY_PHYSICAL) return go_rigid(k_nonpressure_rigid<SPHX_VISCOSITY_PHYSICAL>, ViscArg<SPHX_VISCOSITY_PHYSICAL>{c->VK});
            go_rigid(k_nonpressure_rigid<SPHX_VISCOSITY_XSPH>, ViscArg<SPHX_VISCOSITY_XSPH>{});
        }, false);
    }
    c->accel_uniform.filled();  // (the full pass writes every acceleration)
    auto go = [&](auto kernel, auto visc) {
        hipLaunchKernelGGL(kernel, dim3(nblocks(n)), dim3(256), 0, c->stream, c->pv(), (const float*)c->density, n, c->soff(), c->K, dt_prev, c->nbv(), c->accel,
                           c->d_scal, vslot, visc);
        if (judged) hipLaunchKernelGGL(k_rigid_judge, dim3(1), dim3(64), 0, c->stream, (const DevScalars*)c->d_scal, c->K.rho0, dt_prev, ra);
    };
    launch(c, "nonpressure_accel_vmax", (16.0 + 8 + 4 + list_bytes(c)) * n, [&] {
        if (c->VK.visc_model == SPHX_VISCOSITY_PHYSICAL) return go(k_nonpressure<SPHX_VISCOSITY_PHYSICAL>, ViscArg<SPHX_VISCOSITY_PHYSICAL>{c->VK});
        go(k_nonpressure<SPHX_VISCOSITY_XSPH>, ViscArg<SPHX_VISCOSITY_XSPH>{});
    });
}

// Run-ahead (sphx_ctx::ahead): the NEXT step's non-pressure pass, with dt_prev = the step that is being finished, goes behind what is
// on the stream.  publish (tile sub-steps): its maximum is published under a mailbox sequence number of its own, taken once the pass
// is queued; the single context's pass is published by the sphx_step_begin_law that adopts it.
void enqueue_run_ahead(sphx_ctx* c, float dt, bool publish) {
    const uint32_t vslot = take_vmax_slot(c);
    c->ahead.queued = c->ahead.valid = true;
    c->ahead.vslot = vslot;
    c->ahead.seq = 0;
    c->ahead.n = c->N;
    std::memcpy(&c->ahead.dt_bits, &dt, 4);
    enqueue_nonpressure(c, dt, vslot, publish ? VelMarks::Taken{} : c->velmarks.take());  // (publish: a tile sub-step)
    if (publish) {
        c->ahead.seq = ++c->seq;
        hipLaunchKernelGGL(k_publish_vmax, dim3(1), dim3(64), 0, c->stream, c->d_scal, VmaxArgs{1u, vslot, c->mbox_dev, c->ahead.seq});
    }
}

// One solver loop (dfsph.rs:195-247 density / :346-402 divergence).  pre_seq != 0: `pre_q` iterations (the first one publishing
// pre_seq) of loop generation pre_gen are already on the stream.  count_ok: see enqueue_context_iteration.
// run_ahead (last loop of a step only): see sphx_ctx::ahead.
int solver_loop(sphx_ctx* c, bool divergence, float dt, uint32_t* out_iters, float* out_avg, uint32_t* out_warm, uint32_t* io_flags, bool count_ok,
                uint32_t pre_seq = 0, uint32_t pre_q = 0, uint32_t pre_gen = 0, bool run_ahead = false) {
    uint32_t iters = 0;
    float avg = 0;
    int rc;
    if (device_loop(c)) {
        // The device applies the residual test itself; the host only keeps enough iterations on the stream.  As many as the previous
        // step needed are queued up front (the count changes slowly): in the steady state the loop runs without a single host round
        // trip, an iteration too many costs two kernels that return at once, one too few costs one round trip.
        const uint32_t prev = std::max(1u, divergence ? c->num_divergence_iters : c->num_density_iters);
        const uint32_t cap = (divergence ? c->P.max_divergence_iterations : c->P.max_density_iterations) + 1;
        uint32_t gen = pre_gen, q = pre_q, seq1 = pre_seq;  // seq1: mailbox sequence of iteration 1 (iteration k publishes seq1 + k - 1)
        if (!pre_seq) {
            if (++c->loop_gen == 0) c->loop_gen = 1;
            gen = c->loop_gen;
            seq1 = enqueue_context_iteration(c, divergence, dt, nullptr, 1, gen, out_warm, count_ok);
            q = 1;
        }
        while (q < std::min(prev, cap)) enqueue_context_iteration(c, divergence, dt, nullptr, ++q, gen, out_warm, count_ok);
        if (run_ahead && c->run_ahead) enqueue_run_ahead(c, dt, false);
        uint32_t w = q;  // the iteration whose verdict the host waits for: the last predicted one first
        for (;;) {
            bool done = false;
            if ((rc = wait_loop(c, seq1 + w - 1, gen, &done))) return rc;
            if (done) break;
            c->ahead.valid = false;  // more iterations follow: the pass queued above has read velocities that were not final
            // iteration w has published without meeting the test: the prediction was too low.  From here on keep one full iteration
            // queued behind the one that is running (the host then never sits on the device's critical path).
            while (q < w + 2) enqueue_context_iteration(c, divergence, dt, nullptr, ++q, gen, out_warm, count_ok);
            w += 1;
        }
        iters = c->mbox->loop_iters;
        // the terminating iteration's publish (flags, counters) is complete once ITS seq has arrived
        if ((rc = wait_mailbox(c, seq1 + iters - 1))) return rc;
        // the hint for this loop's next corrections: the terminating one (launched with flags) saw no mark of its iteration
        c->quiet_hint[divergence ? 1 : 0] = c->mbox->quiet_seq == seq1 + iters - 1;
        // Verify every decision the device took, bit for bit, from the residual sums it left in the mailbox.
        const uint32_t first = iters > LOOP_HIST - 1 ? iters - (LOOP_HIST - 1) : 1;
        for (uint32_t k = first; k <= iters; ++k) {
            bool more;
            uint32_t fl = 0;
            if ((rc = judge_residual(c, divergence, c->mbox->loop_hist[k % LOOP_HIST], k, dt, &avg, &more, &fl))) return rc;
            if (more != (k < iters)) {
                c->uploaded = false;
                return c->fail(SPHX_ERR_HIP, "the device's residual test disagrees with the host's (solver loop); upload the state again");
            }
            if (k == iters) *io_flags |= fl;
        }
    } else {
        uint32_t seq = pre_seq ? pre_seq : enqueue_context_iteration(c, divergence, dt, nullptr, 1, 0, out_warm, count_ok);
        for (;;) {
            iters += 1;
            // the residual was published by compute_error; the correction kernel runs while the host reads it
            if ((rc = wait_mailbox(c, seq))) return rc;
            bool more;
            if ((rc = judge_residual(c, divergence, c->mbox->err_sum, iters, dt, &avg, &more, io_flags))) return rc;
            if (!more) {
                c->quiet_hint[divergence ? 1 : 0] = c->mbox->quiet_seq == seq;
                break;
            }
            seq = enqueue_context_iteration(c, divergence, dt, nullptr, iters + 1, 0, out_warm, count_ok);
        }
    }
    *out_iters = iters;
    *out_avg = avg;
    if (divergence)
        c->num_divergence_iters = iters;
    else
        c->num_density_iters = iters;
    return SPHX_OK;
}

}  // namespace

// ======================================================================================================================
// C ABI
// ======================================================================================================================
extern "C" {

uint32_t sphx_abi_version(void) { return SPHX_ABI_VERSION; }

int sphx_default_params(float smoothing_factor, float particle_density, float fluid_density, sphx_params* p) {
    if (!p || !(particle_density > 0)) return SPHX_ERR_INVALID_ARGUMENT;
    std::memset(p, 0, sizeof(*p));
    const float radius = 0.5f / std::sqrt(particle_density);           // fluidparticleworld.rs:82-85
    p->smoothing_length = 2.0f * radius * smoothing_factor;            // fluidparticleworld.rs:58
    p->particle_mass = fluid_density / particle_density;               // fluidparticleworld.rs:74-76
    p->fluid_density = fluid_density;
    p->particle_radius = radius;
    p->gravity[0] = 0.0f;                                              // fluidparticleworld.rs:123
    p->gravity[1] = -9.81f;
    p->grid_min[0] = -100.0f;                                          // neighborhood_search.rs:478
    p->grid_min[1] = -100.0f;
    p->xsph_epsilon = 0.05f;                                           // xsph.rs:14
    p->viscosity_model = SPHX_VISCOSITY_XSPH;                          // main.rs:99-100: DFSPHSolver::new(xsphviscosity, ..)
    p->fluid_viscosity = 1.0016f / 1000.0f;                            // physical.rs:14 (water at 20 degrees)
    p->max_avg_density_error = 0.01f / 100.0f;                         // dfsph.rs:49
    p->max_density_iterations = 200;                                   // dfsph.rs:50
    p->max_divergence_error = 0.1f / 100.0f;                           // dfsph.rs:53
    p->max_divergence_iterations = 400;                                // dfsph.rs:54
    p->device = 0;
    return SPHX_OK;
}

const char* sphx_last_error(const sphx_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int sphx_debug_correction_counts(sphx_ctx* c, uint64_t out[3]) {
    if (!c || !out) return SPHX_ERR_INVALID_ARGUMENT;
    SPHX_HIP(c, hipSetDevice(c->device));
    SPHX_HIP(c, hipStreamSynchronize(c->stream));
    std::vector<Stripe> st(STRIPES);
    SPHX_HIP(c, hipMemcpy(st.data(), c->d_scal->stripe, sizeof(Stripe) * STRIPES, hipMemcpyDeviceToHost));
    out[0] = out[1] = out[2] = 0;
    for (const Stripe& s : st) {
        out[0] += s.zs_skipped;
        out[1] += s.zs_window;
        out[2] += s.zs_remote;
    }
    return SPHX_OK;
}

int sphx_debug_takeover_counts(sphx_ctx* c, uint64_t out[3]) {
    if (!c || !out) return SPHX_ERR_INVALID_ARGUMENT;
    out[0] = c->thin_launches;
    out[1] = c->takeover_producers;
    SPHX_HIP(c, hipSetDevice(c->device));
    SPHX_HIP(c, hipStreamSynchronize(c->stream));
    unsigned long long moved = 0;
    SPHX_HIP(c, hipMemcpy(&moved, &c->d_scal->spec.moved, sizeof(moved), hipMemcpyDeviceToHost));
    out[2] = moved;
    return SPHX_OK;
}

int sphx_debug_rigid_counts(sphx_ctx* c, uint64_t out[3]) {
    if (!c || !out) return SPHX_ERR_INVALID_ARGUMENT;
    out[0] = c->rigid_launches;
    SPHX_HIP(c, hipSetDevice(c->device));
    SPHX_HIP(c, hipStreamSynchronize(c->stream));
    uint32_t dev[2] = {0u, 0u};
    SPHX_HIP(c, hipMemcpy(dev, &c->d_scal->rigid_exits, sizeof(dev), hipMemcpyDeviceToHost));
    out[1] = dev[0];
    out[2] = dev[1];
    return SPHX_OK;
}

int sphx_debug_rigid_predict_counts(sphx_ctx* c, uint64_t out[4]) {
    if (!c || !out) return SPHX_ERR_INVALID_ARGUMENT;
    SPHX_HIP(c, hipSetDevice(c->device));
    SPHX_HIP(c, hipStreamSynchronize(c->stream));
    std::vector<Stripe> st(STRIPES);
    SPHX_HIP(c, hipMemcpy(st.data(), c->d_scal->stripe, sizeof(Stripe) * STRIPES, hipMemcpyDeviceToHost));
    out[0] = c->rigid_predict_launches;
    out[1] = out[2] = out[3] = 0;
    for (const Stripe& s : st) {
        out[1] += s.rp_exit;
        out[2] += s.rp_walk;
        out[3] += s.rp_noverdict;
    }
    return SPHX_OK;
}

int sphx_debug_download_accel(sphx_ctx* c, float* out_xy) {
    if (!c || (c->N && !out_xy)) return SPHX_ERR_INVALID_ARGUMENT;
    SPHX_HIP(c, hipSetDevice(c->device));
    read_accel(c);  // (a rigid pass leaves the array to its reader: the fill comes first; the course of the run does not change)
    SPHX_HIP(c, hipStreamSynchronize(c->stream));
    if (c->N) SPHX_HIP(c, hipMemcpy(out_xy, c->accel, (size_t)c->N * 8, hipMemcpyDeviceToHost));
    return SPHX_OK;
}

int sphx_debug_quiet_counts(sphx_ctx* c, uint64_t out[2]) {
    if (!c || !out) return SPHX_ERR_INVALID_ARGUMENT;
    SPHX_HIP(c, hipSetDevice(c->device));
    SPHX_HIP(c, hipStreamSynchronize(c->stream));
    std::vector<Stripe> st(STRIPES);
    SPHX_HIP(c, hipMemcpy(st.data(), c->d_scal->stripe, sizeof(Stripe) * STRIPES, hipMemcpyDeviceToHost));
    out[0] = 0;
    for (const Stripe& s : st) out[0] += s.zs_quiet;
    out[1] = c->qf_launches;
    return SPHX_OK;
}

int sphx_create(const sphx_params* params, sphx_ctx** out) {
    if (!params || !out) return SPHX_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    if (!(params->smoothing_length > 0) || !(params->particle_mass > 0) || !(params->fluid_density > 0)) {
        g_create_error = "smoothing_length, particle_mass and fluid_density must be positive";
        return SPHX_ERR_INVALID_ARGUMENT;
    }
    if (params->viscosity_model != SPHX_VISCOSITY_XSPH && params->viscosity_model != SPHX_VISCOSITY_PHYSICAL) {
        g_create_error = "viscosity_model must be SPHX_VISCOSITY_XSPH (0) or SPHX_VISCOSITY_PHYSICAL (1)";
        return SPHX_ERR_INVALID_ARGUMENT;
    }
    if (!std::isfinite(params->fluid_viscosity)) {  // (negative values are accepted, as PhysicalViscosityModel does)
        g_create_error = "fluid_viscosity must be finite";
        return SPHX_ERR_INVALID_ARGUMENT;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || params->device < 0 || params->device >= ndev) {
        g_create_error = "no usable HIP device (libsphx has no CPU fallback)";
        return SPHX_ERR_NO_DEVICE;
    }
    sphx_ctx* c = new sphx_ctx();
    if (const char* e = std::getenv("SPHX_SCAN_TWO_PASS")) c->scan_two_pass = e[0] == '1';
    if (const char* e = std::getenv("SPHX_NO_FUSED_COUNT")) c->no_fused_count = e[0] == '1';
    if (const char* e = std::getenv("SPHX_HOST_LOOP")) c->host_loop = e[0] == '1';
    if (const char* e = std::getenv("SPHX_RUN_AHEAD")) c->run_ahead = e[0] != '0';
    if (const char* e = std::getenv("SPHX_FUSE_PREDICT")) c->fuse_predict = e[0] != '0';
    if (const char* e = std::getenv("SPHX_LAZY_TABLE")) c->lazy_table = e[0] != '0' ? 1 : 0;
    if (const char* e = std::getenv("SPHX_STREAM_LISTS")) c->stream_lists = e[0] != '0' ? 1 : 0;
    if (const char* e = std::getenv("SPHX_NT_COLD_STORES")) c->nt_cold_stores = e[0] != '0' ? 1 : 0;
    if (const char* e = std::getenv("SPHX_TILE_FUSE_CLASS")) c->tile_fuse_class = e[0] != '0';
    if (const char* e = std::getenv("SPHX_FUSE_DIV")) c->fuse_div = e[0] != '0';
    if (const char* e = std::getenv("SPHX_XCD_CHUNK")) c->xcd_chunk = (int)xcd_shift_clamp(std::atoi(e));  // log2(blocks per chunk); 0: contiguous eighths
    if (const char* e = std::getenv("SPHX_ALTERNATE_SWEEP")) c->alternate_sweep = e[0] == '2' ? 2 : (e[0] != '0');  // (0: every launch bottom-up; 2: the scatter toggles too — A/B forms)
    if (const char* e = std::getenv("SPHX_ZERO_SKIP")) c->zero_skip = e[0] != '0';  // (0: no correction skips its walk, no flags are written; 1: also below 4 M particles)
    if (const char* e = std::getenv("SPHX_ZERO_SKIP_COUNT")) c->zero_skip_count = e[0] == '1';  // (test aid: sphx_debug_correction_counts)
    if (const char* e = std::getenv("SPHX_QUIET_TAKEOVER")) c->quiet_takeover = std::strcmp(e, "force") == 0 ? 2 : (e[0] != '0' ? 1 : 0);  // (0: the A/B switch)
    if (const char* e = std::getenv("SPHX_QUIET_TAKEOVER_DENSITY")) c->quiet_takeover_density = e[0] != '0';  // (0: divergence loop only — the per-part A/B)
    if (const char* e = std::getenv("SPHX_RIGID_SKIP")) c->rigid_skip = std::strcmp(e, "force") == 0 ? 2 : (e[0] != '0' ? 1 : 0);  // (0: the A/B switch; unset: from 4 M particles)
    if (const char* e = std::getenv("SPHX_RIGID_PREDICT")) c->rigid_predict = std::strcmp(e, "accel") == 0 ? 1 : (e[0] != '0' ? 2 : 0);  // (0: the A/B switch; accel: the per-part A/B)
    if (const char* e = std::getenv("SPHX_THIN_GRID")) c->thin_grid = (uint32_t)std::max(0, std::atoi(e));  // (test aid: small scenes run the block loop)
    if (const char* e = std::getenv("SPHX_FUSE_WARM")) c->fuse_warm = e[0] != '0';  // (A/B: the divergence warm start as a walk of its own behind k_neighbor_build<1>)
    c->P = *params;
    c->device = params->device;
    const float h = params->smoothing_length;
    const float PI_F = (float)3.14159265358979323846;
    Consts& K = c->K;
    K.h = h;
    K.radius_sq = h * h;
    K.cell_inv = 1.0f / h;
    K.gmin_x = params->grid_min[0];
    K.gmin_y = params->grid_min[1];
    K.w_hinv = 1.0f / h;
    K.w_norm = 4.0f * 7.0f / (PI_F * rs_powi(h, 2));
    K.w_ngrad = 140.0f / (PI_F * rs_powi(h, 4));
    K.p6_hsq = h * h;
    K.p6_norm = 4.0f / (PI_F * rs_powi(h, 8));
    K.p6_ngrad = 24.0f / (PI_F * rs_powi(h, 8));
    K.sp_h = h;
    K.sp_norm = 10.0f / (PI_F * rs_powi(h, 5));
    K.sp_ngrad = 30.0f / (PI_F * rs_powi(h, 5));
    K.mass = params->particle_mass;
    K.rho0 = params->fluid_density;
    K.xsph_eps = params->xsph_epsilon;
    c->VK.visc_model = params->viscosity_model;
    c->VK.mu = params->fluid_viscosity;
    c->VK.vis_nlap = 360.0f / (29.0f * PI_F * rs_powi(h, 5));  // Viscosity::new, viscosity.rs:24: (29 pi) h^5 in f32, powi as compiler-rt
    K.tile = TileRect{0u, 65536u, 0u, 65536u};
    K.remote_cap = params->list_span_limit == SPHX_LISTS_32BIT ? 0u : params->list_span_limit == 0 ? REMOTE_CAP : std::min(params->list_span_limit, REMOTE_CAP);
    {
        // every list entry has d2 <= fl(h h), so r = sqrt(d2) <= sqrt(fl(h h)) (= h: checked, not assumed) and q = fl(r * w_hinv) <=
        // fl(h * w_hinv): when that is <= 1 the kernel's min(q, 1) never changes a value (SPHX_QCLAMP=1 keeps it for A/B runs)
        volatile float hh = h * h, root = std::sqrt(hh), qmax = h * K.w_hinv;
        c->fast_walk_ok = (root == h && qmax <= 1.0f) ? 1u : 0u;
        if (const char* e = std::getenv("SPHX_QCLAMP")) if (e[0] == '1') c->fast_walk_ok = 0u;
        // ... and the lists have to belong to the positions: K.q_noclamp is raised by the neighbour build (update_neighborhood) and
        // dropped by whatever replaces positions behind the lists' back (lists_went_stale)
        K.q_noclamp = 0u;
        K.rev = 0u;
        K.nt_cold = 0u;
        K.xcd_shift = 0u;
    }
    K.gx = params->gravity[0];
    K.gy = params->gravity[1];
    {  // WCSPHSolver::new -> set_compressibility(props, 0.01, 1.0), wscsph.rs:31-49
        const float speed_of_sound = 1.0f / std::sqrt(0.01f);
        K.wc_stiffness = params->fluid_density * speed_of_sound * speed_of_sound / 7.0f;
        K.wc_boundary_force = 1.0f;
    }
    K.ax = params->gravity[0] * K.mass / K.mass;  // dfsph.rs:442-444
    K.ay = params->gravity[1] * K.mass / K.mass;
    auto bail = [&](const char* what, hipError_t e) {
        g_create_error = std::string(what) + ": " + hipGetErrorString(e);
        sphx_destroy(c);  // frees whatever exists so far (stream, scalars, mailbox)
        return SPHX_ERR_HIP;
    };
    hipError_t e;
    if ((e = hipSetDevice(c->device)) != hipSuccess) return bail("hipSetDevice", e);
    if ((e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking)) != hipSuccess) return bail("hipStreamCreate", e);
    if ((e = hipMalloc((void**)&c->d_scal, sizeof(DevScalars))) != hipSuccess) return bail("hipMalloc", e);
    if ((e = hipHostMalloc((void**)&c->mbox, sizeof(Mailbox), hipHostMallocMapped | hipHostMallocCoherent)) != hipSuccess)
        return bail("hipHostMalloc", e);
    std::memset((void*)c->mbox, 0, sizeof(Mailbox));
    if ((e = hipHostGetDevicePointer((void**)&c->mbox_dev, (void*)c->mbox, 0)) != hipSuccess) return bail("hipHostGetDevicePointer", e);
    if ((e = hipMemsetAsync(c->d_scal, 0, sizeof(DevScalars), c->stream)) != hipSuccess) return bail("hipMemset", e);
    // empty grids + empty [N|B] arrays so neighbour builds work before any boundary / particle is set
    int rc = set_directory(c, c->gdyn, 0, 0, 0, 0, nullptr, true);
    if (!rc) rc = set_directory(c, c->gstat, 0, 0, 0, 0, nullptr, true);
    if (!rc) rc = dev_alloc(c, &c->bpos, 1);
    if (!rc) rc = dev_alloc(c, &c->bpos2, 1);
    if (!rc) rc = dev_alloc(c, &c->bid, 1);
    if (!rc) rc = dev_alloc(c, &c->bid2, 1);
    if (!rc) rc = ensure_nb_arrays(c, 0, 1, false);
    if (rc) {
        g_create_error = c->err;
        sphx_destroy(c);
        return rc;
    }
    c->capB = 1;
    *out = c;
    return SPHX_OK;
}

void sphx_destroy(sphx_ctx* c) {
    if (!c) return;
    hipSetDevice(c->device);
    if (c->stream) hipStreamSynchronize(c->stream);
#ifdef SPHX_STAMPS
    {
        unsigned long long h[4][16];
        if (hipMemcpyFromSymbol(h, HIP_SYMBOL(sphx::g_stamp), sizeof(h)) == hipSuccess)
            for (int m = 0; m < 4; ++m) {
                if (!h[m][15]) continue;
                std::fprintf(stderr, "SPHX_STAMPS build<%d> waves=%llu cycles/wave:", m, h[m][15]);
                for (int k = 0; k < 8; ++k) std::fprintf(stderr, " p%d=%.0f", k, (double)h[m][k] / (double)h[m][15]);
                // SPHX_STAMP_VMWAIT pairs {cycles, occurrences}: 8 scan, prefetched first trips; 10 scan, blocking trips; 12 second walk
                for (int k = 8; k < 14; k += 2)
                    std::fprintf(stderr, " w%d=%.0f/%.2f", k, h[m][k + 1] ? (double)h[m][k] / (double)h[m][k + 1] : 0.0, (double)h[m][k + 1] / (double)h[m][15]);
                std::fprintf(stderr, "\n");
            }
    }
#endif
    for (auto& p : c->prof_pending) {
        hipEventDestroy(p.a);
        hipEventDestroy(p.b);
    }
    for (auto e : c->ev_pool) hipEventDestroy(e);
    dev_free(&c->posA); dev_free(&c->posA2); dev_free(&c->vel); dev_free(&c->vel2); dev_free(&c->kbuf); dev_free(&c->knz); dev_free(&c->accel);
    dev_free(&c->density); dev_free(&c->alpha); dev_free(&c->alpha2); dev_free(&c->kappa); dev_free(&c->stiff); dev_free(&c->kappa2); dev_free(&c->stiff2);
    dev_free(&c->pid); dev_free(&c->pid2); dev_free(&c->key); dev_free(&c->order);
    dev_free(&c->bpos); dev_free(&c->bpos2); dev_free(&c->bid); dev_free(&c->bid2); dev_free(&c->nb_list); dev_free(&c->nb_wave); dev_free(&c->nb_counts); dev_free(&c->nb_remote);
    dev_free(&c->scan_partials); dev_free(&c->scan_state); dev_free(&c->d_scal); dev_free(&c->tile_blk); dev_free(&c->sample_buf); dev_free(&c->render_buf); dev_free(&c->edit_buf); dev_free(&c->state_dig); dev_free(&c->mstate_buf);
    dev_free(&c->track.set_buf); dev_free(&c->track.rec); dev_free(&c->track.scratch); dev_free(&c->fields_buf);
    dev_free(&c->stats.scratch); dev_free(&c->stats.rec); dev_free(&c->probe.scratch); dev_free(&c->probe.fixed); dev_free(&c->probe.rec); dev_free(&c->tsample.null_grid); dev_free(&c->contour_buf); dev_free(&c->query_buf); dev_free(&c->query_ent);
    free_grid(c->gdyn);
    free_grid(c->gstat);
    if (c->mbox) hipHostFree((void*)c->mbox);
    if (c->view_stream) {
        hipStreamSynchronize(c->view_stream);
        hipEventDestroy(c->view_packed);
        hipEventDestroy(c->view_done);
        hipStreamDestroy(c->view_stream);
        if (c->view_dev) hipFree(c->view_dev);
        if (c->view_host) hipHostFree(c->view_host);
    }
    if (c->stream && !c->external_stream) hipStreamDestroy(c->stream);
    delete c;
}

uint32_t sphx_num_particles(const sphx_ctx* c) { return c ? c->N : 0; }
uint32_t sphx_num_boundary(const sphx_ctx* c) { return c ? c->B : 0; }

// Run on a stream owned by the caller (e.g. the HIP stream behind a torch.cuda.Stream): work of this context and the caller's
// own work on that stream — RCCL sends/receives of the halo buffers — are then ordered by the stream, no host synchronisation.
int sphx_build_stats(const sphx_ctx* c, uint32_t* out_particles, uint64_t* out_entries, uint64_t* out_remote) {
    if (!c) return SPHX_ERR_INVALID_ARGUMENT;
    if (out_particles) *out_particles = c->N;
    if (out_entries) *out_entries = c->nb_last;
    if (out_remote) *out_remote = c->rem_last;
    return SPHX_OK;
}

int sphx_set_stream(sphx_ctx* c, void* hip_stream) {
    if (!c) return SPHX_ERR_INVALID_ARGUMENT;
    c->ahead.valid = false;
    if (c->in_step) return c->fail(SPHX_ERR_NOT_READY, "sphx_set_stream inside a step");
    SPHX_HIP(c, hipSetDevice(c->device));
    SPHX_HIP(c, hipStreamSynchronize(c->stream));
    if (c->stream && !c->external_stream) hipStreamDestroy(c->stream);
    if (hip_stream) {
        c->stream = (hipStream_t)hip_stream;
        c->external_stream = true;
    } else {
        SPHX_HIP(c, hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
        c->external_stream = false;
    }
    return SPHX_OK;
}

int sphx_synchronize(sphx_ctx* c) {
    if (!c) return SPHX_ERR_INVALID_ARGUMENT;
    SPHX_HIP(c, hipSetDevice(c->device));
    SPHX_HIP(c, hipStreamSynchronize(c->stream));
    return SPHX_OK;
}

int sphx_set_boundary(sphx_ctx* c, const float* xy, uint32_t n) {
    if (!c || (n && !xy)) return SPHX_ERR_INVALID_ARGUMENT;
    c->ahead.valid = false;
    if (c->in_step) return c->fail(SPHX_ERR_NOT_READY, "sphx_set_boundary between step_begin and step_finish");
    sample_went_stale(c, "sphx_set_boundary replaced the boundary (its grid is rebuilt by the next neighbour build): run a step, or "
                         "sphx_update_neighborhood + sphx_update_densities");
    SPHX_HIP(c, hipSetDevice(c->device));
    int rc;
    if (n > c->capB) {
        SPHX_HIP(c, hipStreamSynchronize(c->stream));
        if ((rc = dev_alloc(c, &c->bpos, n)) || (rc = dev_alloc(c, &c->bpos2, n)) || (rc = dev_alloc(c, &c->bid, n)) ||
            (rc = dev_alloc(c, &c->bid2, n)))
            return rc;
        if ((rc = ensure_nb_arrays(c, c->capN, n, true))) return rc;
        c->capB = n;
    }
    c->B = n;
    if (n) {
        SPHX_HIP(c, hipMemcpyAsync(c->bpos, xy, (size_t)n * 8, hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(k_iota, dim3(nblocks(n)), dim3(256), 0, c->stream, c->bid, n);
        SPHX_HIP(c, hipStreamSynchronize(c->stream));
    }
    c->h_boundary.assign(xy, xy + 2 * (size_t)n);
    c->quiet_hint[0] = c->quiet_hint[1] = false;
    c->rigid_forget();
    c->boundary_changed = true;  // fluidparticleworld.rs:194 (the static grid is rebuilt lazily, :247-252)
    return ensure_index_scratch(c);
}

int sphx_upload(sphx_ctx* c, const float* pos_xy, const float* vel_xy, uint32_t n) {
    if (!c || (n && !pos_xy)) return SPHX_ERR_INVALID_ARGUMENT;
    c->ahead.valid = false;
    if (c->in_step) return c->fail(SPHX_ERR_NOT_READY, "sphx_upload between step_begin and step_finish");
    // (first: a failed reallocation below leaves the particle arrays freed)
    sample_went_stale(c, "sphx_upload replaced the particles: run a step, or sphx_update_neighborhood + sphx_update_densities");
    SPHX_HIP(c, hipSetDevice(c->device));
    SPHX_HIP(c, hipStreamSynchronize(c->stream));
    clear_histograms(c);
    int rc;
    if ((rc = alloc_particles(c, n))) return rc;
    c->N = n;
    c->ids_issued = n;  // particle_id = index in this upload; sphx_append continues from here
    c->set_changed = false;
    lists_went_stale(c);
    if (n) {
        SPHX_HIP(c, hipMemcpyAsync(c->posA, pos_xy, (size_t)n * 8, hipMemcpyHostToDevice, c->stream));
        if (vel_xy)
            SPHX_HIP(c, hipMemcpyAsync(c->vel, vel_xy, (size_t)n * 8, hipMemcpyHostToDevice, c->stream));
        else
            SPHX_HIP(c, hipMemsetAsync(c->vel, 0, (size_t)n * 8, c->stream));
        hipLaunchKernelGGL(k_iota, dim3(nblocks(n)), dim3(256), 0, c->stream, c->pid, n);
        SPHX_HIP(c, hipStreamSynchronize(c->stream));
    }
    c->have_fluid_bbox = cell_bbox(c, pos_xy, n, c->fb);
    c->uploaded = true;
    // a fresh upload is a fresh scene: cover its blocks only (coverage otherwise only ever grows)
    c->gdyn.cover.clear();
    c->gdyn.nbx = c->gdyn.nby = 0;
    if (c->have_fluid_bbox && (rc = cover_dynamic(c, pos_xy, n, false))) return rc;
    return ensure_index_scratch(c);
}

int sphx_clear_cached(sphx_ctx* c) {  // dfsph.rs:406-412
    if (!c) return SPHX_ERR_INVALID_ARGUMENT;
    c->ahead.valid = false;
    if (c->in_step) return c->fail(SPHX_ERR_NOT_READY, "sphx_clear_cached between step_begin and step_finish");
    SPHX_HIP(c, hipSetDevice(c->device));
    c->cached_n = 0;
    c->num_divergence_iters = 0;
    c->num_density_iters = 0;
    c->wcsph_n = 0;  // WCSPHSolver::clear_cached_data: accellerations.clear() (wscsph.rs:122-124)
    if (c->capN) {
        SPHX_HIP(c, hipMemsetAsync(c->kappa, 0, (size_t)c->capN * 4, c->stream));
        SPHX_HIP(c, hipMemsetAsync(c->stiff, 0, (size_t)c->capN * 4, c->stream));
        SPHX_HIP(c, hipMemsetAsync(c->alpha, 0, (size_t)c->capN * 4, c->stream));
    }
    return SPHX_OK;
}

int sphx_update_neighborhood(sphx_ctx* c) {
    if (!c) return SPHX_ERR_INVALID_ARGUMENT;
    c->ahead.valid = false;
    if (!c->uploaded) return c->fail(SPHX_ERR_NOT_READY, "no particles uploaded");
    if (c->in_step) return c->fail(SPHX_ERR_NOT_READY, "sphx_update_neighborhood between step_begin and step_finish");
    SPHX_HIP(c, hipSetDevice(c->device));
    int rc = update_neighborhood(c, false, 0.0f, false);
    if (rc) return rc;
    return publish_and_wait(c);
}

int sphx_update_densities(sphx_ctx* c, int kind) {
    if (!c) return SPHX_ERR_INVALID_ARGUMENT;
    c->ahead.valid = false;
    if (!c->uploaded) return c->fail(SPHX_ERR_NOT_READY, "no particles uploaded");
    SPHX_HIP(c, hipSetDevice(c->device));
    if (kind == SPHX_KERNEL_WENDLAND_C2)
        launch_density<0>(c, true, false);
    else if (kind == SPHX_KERNEL_POLY6)
        launch_density<1>(c, true, false);
    else if (kind == SPHX_KERNEL_SPIKY)
        launch_density<2>(c, true, false);
    else
        return c->fail(SPHX_ERR_INVALID_ARGUMENT, "unknown kernel kind");
    if (c->sample_ready == 1u) c->sample_ready = 2u;  // a neighbour build plus its densities: the fields may be sampled
    return SPHX_OK;
}

int sphx_compute_alpha(sphx_ctx* c) {
    if (!c) return SPHX_ERR_INVALID_ARGUMENT;
    c->ahead.valid = false;
    if (!c->uploaded) return c->fail(SPHX_ERR_NOT_READY, "no particles uploaded");
    SPHX_HIP(c, hipSetDevice(c->device));
    launch_density<0>(c, false, true);
    return SPHX_OK;
}

int sphx_step_begin_law(sphx_ctx* c, float dt_prev, const sphx_timer_law* law, float* out_vmax) {
    if (!c || !out_vmax) return SPHX_ERR_INVALID_ARGUMENT;
    if (!c->uploaded) return c->fail(SPHX_ERR_NOT_READY, "sphx_step_begin before sphx_upload");
    if (c->in_step) return c->fail(SPHX_ERR_NOT_READY, "sphx_step_begin called twice");
    if (!(dt_prev > 0) || !std::isfinite(dt_prev)) return c->fail(SPHX_ERR_INVALID_ARGUMENT, "dt_prev must be positive and finite");
    if (law && (law->timestep_min_ns > law->timestep_max_ns || !(law->particle_diameter > 0) || !(law->cfl_factor > 0) || law->simulation_step_ns == 0))
        return c->fail(SPHX_ERR_INVALID_ARGUMENT, "sphx_timer_law: need 0 < min <= max, a positive diameter, cfl factor and current step");
    SPHX_HIP(c, hipSetDevice(c->device));
    sample_went_stale(c, "the last DFSPH step did not finish: run a step, or sphx_update_neighborhood + sphx_update_densities");
    const bool ahead_ok = c->ahead.queued && c->ahead.valid;
    c->ahead.valid = false;
    c->step_flags = 0;
    c->step_dt_prev = dt_prev;
    c->pre_seq = 0;
    c->law_active = false;
    const uint32_t n = c->N;
    int rc;
    if (c->cached_n != n || c->set_changed) {  // warm-up, dfsph.rs:419-428 (set_changed: sphx_append / sphx_remove since the last one)
        c->set_changed = false;
        if (n > c->cached_n) {
            const uint32_t add = n - c->cached_n;
            for (float* a : {c->alpha, c->kappa, c->stiff})
                hipLaunchKernelGGL(k_fill_f32, dim3(nblocks(add)), dim3(256), 0, c->stream, a, c->cached_n, n, 0.0f);
        }
        c->cached_n = n;
        if ((rc = update_neighborhood(c, true, 0.0f, true))) return rc;  // regrid (alpha permuted), densities, alpha factors
        c->step_flags |= SPHX_FLAG_WARMUP;
    }
    if (n == 0) {
        *out_vmax = 0.0f;
        c->step_vmax = 0.0f;
        c->in_step = true;
        return SPHX_OK;
    }
    TimerLaw tl{};
    if (law) {
        tl.enabled = 1;
        tl.adaptive = law->adaptive ? 1u : 0u;
        tl.cfl_factor = law->cfl_factor;
        tl.particle_diameter = law->particle_diameter;
        tl.min_ns = law->timestep_min_ns;
        tl.max_ns = law->timestep_max_ns;
        tl.step_ns = law->simulation_step_ns;
    }
    const uint32_t seq = ++c->seq;
    uint32_t dt_prev_bits;
    std::memcpy(&dt_prev_bits, &dt_prev, 4);
    // the pass may already be on the stream (queued by the previous sphx_step_finish, sphx_ctx::ahead)
    const bool adopted = ahead_ok && !(c->step_flags & SPHX_FLAG_WARMUP) && c->ahead.n == n && c->ahead.dt_bits == dt_prev_bits;
    uint32_t vslot;
    if (adopted) {
        vslot = c->ahead.vslot;
        c->ahead.queued = false;
    } else {
        vslot = take_vmax_slot(c);
        enqueue_nonpressure(c, dt_prev, vslot);
    }
    const VmaxArgs va{1u, vslot, c->mbox_dev, seq};  // whoever is queued behind the non-pressure pass reads and publishes its maximum
    if (!law) hipLaunchKernelGGL(k_publish_vmax, dim3(1), dim3(64), 0, c->stream, c->d_scal, va);
    if (law) {
        // phase B up to its first decision point goes onto the stream now (dfsph.rs:484-492, first pass of :195-247): the prediction
        // derives dt from the maximum itself and leaves it in device memory for the kernels behind it — the GPU does not idle while
        // the host turns vmax into dt
        const float* dt_dev = &c->d_scal->dt;
        // no warm start in front of the first density iteration (dfsph.rs:199): its compute_density_error does the prediction too
        const bool fuse_pred = c->fuse_predict && c->num_density_iters <= 1;
        PredArgs pa{};
        pa.va = va;
        pa.law = tl;
        const PredArgs* const pred = fuse_pred ? &pa : nullptr;
        if (!fuse_pred)
            launch_predict(c, "velocity_prediction", 1.0f, va, tl);
        if (device_loop(c)) {
            // as many constant-density iterations as the previous step needed, all reading the device's dt; the device stops the loop
            if (++c->loop_gen == 0) c->loop_gen = 1;
            c->pre_gen = c->loop_gen;
            const uint32_t want = std::min(std::max(1u, c->num_density_iters), c->P.max_density_iterations + 1);
            c->pre_seq = enqueue_context_iteration(c, false, 1.0f, dt_dev, 1, c->pre_gen, &c->pre_warm, true, pred);
            for (c->pre_queued = 1; c->pre_queued < want;) enqueue_context_iteration(c, false, 1.0f, dt_dev, ++c->pre_queued, c->pre_gen, &c->pre_warm, true);
        } else {
            c->pre_gen = 0;
            c->pre_queued = 1;
            c->pre_seq = enqueue_context_iteration(c, false, 1.0f, dt_dev, 1, 0, &c->pre_warm, true, pred);
        }
        c->law_active = true;
    }
    if ((rc = wait_mailbox(c, seq))) return rc;
    if (c->rigid_judged) {  // the hint for the next non-pressure launch: the judged one (behind this seq on the stream) saw no mark
        c->rigid_hint = c->mbox->rigid_tag == c->rigid_judged;
        c->rigid_judged = 0;
    }
    const uint32_t vbits = c->mbox->vmax_sq_bits;
    float vsq;
    std::memcpy(&vsq, &vbits, 4);
    if (!std::isfinite(vsq)) return c->fail(SPHX_ERR_NONFINITE, "max velocity is not finite (Duration::from_secs_f32 would panic, timemanager.rs:264)");
    c->step_vmax = std::sqrt(vsq);  // dfsph.rs:479
    c->law_dt_bits = c->mbox->dt_bits;
    *out_vmax = c->step_vmax;
    c->in_step = true;
    return SPHX_OK;
}

int sphx_step_begin(sphx_ctx* c, float dt_prev, float* out_vmax) { return sphx_step_begin_law(c, dt_prev, nullptr, out_vmax); }

// Failure contract of the step: whatever goes wrong, the step is closed (a new sphx_step_begin is accepted).  After a device-side
// failure (SPHX_ERR_HIP, SPHX_ERR_NONFINITE — the reference panics there), or when phase B had already started with a dt the host
// then did not confirm, the device arrays are mid-step garbage: the context asks for a fresh sphx_upload (SPHX_ERR_NOT_READY).
int sphx_step_finish(sphx_ctx* c, float dt, sphx_step_stats* out) {
    if (!c) return SPHX_ERR_INVALID_ARGUMENT;
    if (!c->in_step || c->in_wcsph) return c->fail(SPHX_ERR_NOT_READY, "sphx_step_finish without sphx_step_begin");
    c->in_step = false;
    if (!(dt > 0) || !std::isfinite(dt)) {
        if (c->law_active) c->uploaded = false;  // prediction and the first iterations already ran with the device's own dt
        c->law_active = false;
        drop_fused_count(c);
        return c->fail(SPHX_ERR_INVALID_ARGUMENT, c->uploaded ? "dt must be positive and finite"
                                                               : "dt must be positive and finite (phase B had started: upload the state again)");
    }
    SPHX_HIP(c, hipSetDevice(c->device));
    const uint32_t n = c->N;
    sphx_step_stats s;
    std::memset(&s, 0, sizeof(s));
    s.dt_prev = c->step_dt_prev;
    s.dt = dt;
    s.vmax = c->step_vmax;
    int rc;
    auto broken = [&](int code) {  // the device state is not a consistent particle set any more
        if (code == SPHX_ERR_HIP || code == SPHX_ERR_NONFINITE) {
            c->uploaded = false;
            clear_histograms(c);
        }
        drop_fused_count(c);  // (a count of the next build made by this step's density correction: that build does not come)
        c->ahead.valid = false;
        c->handoff.clear();
        c->rigid_forget();
        c->law_active = false;
        return code;
    };
    if (n) {
        uint32_t pre = 0, pre_q = 0, pre_gen = 0;
        if (c->law_active) {
            uint32_t bits;
            std::memcpy(&bits, &dt, 4);
            if (bits != c->law_dt_bits) {
                // the prediction already ran with the device's dt: the velocities on the device are not the host's any more
                c->uploaded = false;
                c->law_active = false;
                drop_fused_count(c);
                return c->fail(SPHX_ERR_INVALID_ARGUMENT, "dt differs from the sphx_timer_law handed to sphx_step_begin_law; upload the state again");
            }
            pre = c->pre_seq;
            pre_q = c->pre_queued;
            pre_gen = c->pre_gen;
            s.warmstart_density = c->pre_warm;
        } else {
            launch_predict(c, "velocity_prediction", dt);
        }
        c->law_active = false;
        if ((rc = solver_loop(c, false, dt, &s.density_iterations, &s.avg_density_error, &s.warmstart_density, &c->step_flags, true, pre, pre_q, pre_gen)))
            return broken(rc);
        // advect (dfsph.rs:499-510) fused into the re-grid (dfsph.rs:512); densities + alpha (dfsph.rs:516-518) fused into the
        // neighbour build
        // (no warm start in front of the divergence loop <=> the previous one took a single iteration, dfsph.rs:354)
        const bool fuse_div = c->fuse_div && !c->tile_mode && c->num_divergence_iters <= 1;
        const bool fuse_warm = c->fuse_div && c->fuse_warm && !c->tile_mode && c->num_divergence_iters > 1;
        if ((rc = update_neighborhood(c, false, dt, true, fuse_div, fuse_warm))) return broken(rc);
        if ((rc = solver_loop(c, true, dt, &s.divergence_iterations, &s.avg_divergence, &s.warmstart_divergence, &c->step_flags, false, 0, 0, 0, true)))
            return broken(rc);
        // dfsph.rs:524: the predicted velocities in vel[] ARE the new velocities (no copy)
        s.neighbor_entries = c->nb_last;
        s.remote_entries = (uint32_t)std::min<unsigned long long>(c->rem_last, 0xFFFFFFFFull);
    }
    c->law_active = false;
    s.flags = c->step_flags;
    if (out) *out = s;
    sample_after_step(c);  // re-grid, densities (fused into the build) and the divergence loop, which moves no particle
    track_after_step(c);
    stats_after_step(c, dt);
    probe_after_step(c, dt);
    return SPHX_OK;
}

// ---- WCSPHSolver::simulation_step (wscsph.rs:126-179), two-phase like the DFSPH step --------------------------------------------
// phase A: leap frog 1 with dt = time_manager.simulation_step(), re-grid, Poly6 densities, accelerations, max |v + a*dt|
int sphx_wcsph_step_begin(sphx_ctx* c, float dt, float* out_vmax) {
    if (!c || !out_vmax) return SPHX_ERR_INVALID_ARGUMENT;
    c->ahead.valid = false;
    if (!c->uploaded) return c->fail(SPHX_ERR_NOT_READY, "sphx_wcsph_step_begin before sphx_upload");
    if (c->in_step) return c->fail(SPHX_ERR_NOT_READY, "a step is already open");
    if (c->tile_mode) return c->fail(SPHX_ERR_INVALID_ARGUMENT, "WCSPH is not available on tiles");
    if (!(dt > 0) || !std::isfinite(dt)) return c->fail(SPHX_ERR_INVALID_ARGUMENT, "dt must be positive and finite");
    SPHX_HIP(c, hipSetDevice(c->device));
    sample_went_stale(c, "the last WCSPH step did not finish: run a step, or sphx_update_neighborhood + sphx_update_densities");
    c->step_flags = 0;
    c->step_dt_prev = dt;
    const uint32_t n = c->N;
    *out_vmax = 0.0f;
    c->step_vmax = 0.0f;
    if (n == 0) {
        c->in_step = true;
        c->in_wcsph = true;
        return SPHX_OK;
    }
    hipStream_t st = c->stream;
    const dim3 g(nblocks(n)), b(256);
    read_accel(c);  // (leap frog 1 reads accel[]: a DFSPH pass in the rigid form may have left it unwritten)
    if (c->wcsph_n < n)  // accellerations.resize(n, zero), wscsph.rs:129
        SPHX_HIP(c, hipMemsetAsync(c->accel + c->wcsph_n, 0, (size_t)(n - c->wcsph_n) * 8, st));
    c->wcsph_n = n;
    launch(c, "wcsph_leapfrog1", 40.0 * n, [&] { hipLaunchKernelGGL(k_wcsph_leapfrog1, g, b, 0, st, c->vel, c->posA, (const float2*)c->accel, n, dt); });
    // A step whose particles may travel a good part of a 64-cell block (a blow-up: the boundary force of wscsph.rs:109-116 does not
    // scale with the resolution) covers the leap-frogged positions BEFORE the build instead of finding strays in it: a stray is kept
    // without neighbours for that build, which is not the reference's arithmetic.  The estimate is the last step's max |v + a dt|
    // (leap frog 1 adds another half kick: hence the factor 2); a calm run never pays the download.
    if (2.0f * c->wcsph_vmax_prev * dt * c->K.cell_inv > 16.0f) c->recover_streak = std::max(c->recover_streak, 1u);
    int rc;
    if ((rc = update_neighborhood(c, false, 0.0f, false))) return rc;  // update_neighborhood_datastructure(vec![], vec![]), wscsph.rs:152
    launch_density<1>(c, true, false);                                   // update_densities(Poly6), wscsph.rs:153
    const uint32_t seq = ++c->seq;
    const VmaxArgs va{1u, take_vmax_slot(c), c->mbox_dev, seq};
    launch(c, "wcsph_accelerations_vmax", (16.0 + 4 + 8 + 4 + list_bytes(c)) * n, [&] {
        if (c->VK.visc_model == SPHX_VISCOSITY_PHYSICAL)
            hipLaunchKernelGGL(k_wcsph_accel<SPHX_VISCOSITY_PHYSICAL>, g, b, 0, st, c->pv(), (const float*)c->density, n, c->soff(), c->K, dt, c->nbv(),
                               c->accel, c->d_scal, va.vslot, ViscArg<SPHX_VISCOSITY_PHYSICAL>{c->VK});
        else
            hipLaunchKernelGGL(k_wcsph_accel<SPHX_VISCOSITY_XSPH>, g, b, 0, st, c->pv(), (const float*)c->density, n, c->soff(), c->K, dt, c->nbv(),
                               c->accel, c->d_scal, va.vslot, ViscArg<SPHX_VISCOSITY_XSPH>{});
    });
    hipLaunchKernelGGL(k_publish_vmax, dim3(1), dim3(64), 0, st, c->d_scal, va);
    if ((rc = wait_mailbox(c, seq))) return rc;
    const uint32_t vbits = c->mbox->vmax_sq_bits;
    float vsq;
    std::memcpy(&vsq, &vbits, 4);
    if (!std::isfinite(vsq)) return c->fail(SPHX_ERR_NONFINITE, "max velocity is not finite (Duration::from_secs_f32 would panic, timemanager.rs:264)");
    c->step_vmax = std::sqrt(vsq);  // wscsph.rs:163
    c->wcsph_vmax_prev = c->step_vmax;
    *out_vmax = c->step_vmax;
    c->in_step = true;
    c->in_wcsph = true;
    return SPHX_OK;
}

// phase B: leap frog 2 with the dt the timer just returned (wscsph.rs:168-177)
int sphx_wcsph_step_finish(sphx_ctx* c, float dt, sphx_step_stats* out) {
    if (!c) return SPHX_ERR_INVALID_ARGUMENT;
    if (!c->in_step || !c->in_wcsph) return c->fail(SPHX_ERR_NOT_READY, "sphx_wcsph_step_finish without sphx_wcsph_step_begin");
    if (!(dt > 0) || !std::isfinite(dt)) return c->fail(SPHX_ERR_INVALID_ARGUMENT, "dt must be positive and finite");
    SPHX_HIP(c, hipSetDevice(c->device));
    c->in_step = false;
    c->in_wcsph = false;
    const uint32_t n = c->N;
    sphx_step_stats s;
    std::memset(&s, 0, sizeof(s));
    s.dt_prev = c->step_dt_prev;
    s.dt = dt;
    s.vmax = c->step_vmax;
    if (n) {
        launch_predict(c, "wcsph_leapfrog2", 0.5f * dt);  // (the same kernel as the DFSPH prediction)
        int rc = publish_and_wait(c);  // neighbour-entry count and the sticky flags of this step's build
        if (rc) return rc;
        s.neighbor_entries = c->nb_last;
    }
    s.flags = c->step_flags;
    if (out) *out = s;
    sample_after_step(c);  // phase A re-gridded the leap-frogged positions and took their Poly6 densities; leap frog 2 moves none
    track_after_step(c);
    stats_after_step(c, dt);
    probe_after_step(c, dt);
    return SPHX_OK;
}

// ---- viewer feed: strided, asynchronous download (SURVEY.md 8(f) rank 4) ----------------------------------------------------------
// sphx_view_request packs {x, y, |v|} of every stride-th particle on the solver stream and copies it to pinned host memory on a
// separate copy stream: the transfer overlaps the steps that follow.  sphx_view_fetch hands out the pinned buffer of the latest
// completed (wait = 0: or still running -> SPHX_ERR_NOT_READY) request; it stays valid until the next request.
int sphx_view_request(sphx_ctx* c, uint32_t stride, uint32_t* out_count) {
    if (!c || stride == 0) return SPHX_ERR_INVALID_ARGUMENT;
    if (c->in_step) return c->fail(SPHX_ERR_NOT_READY, "sphx_view_request between step_begin and step_finish");
    SPHX_HIP(c, hipSetDevice(c->device));
    const uint32_t n = c->N;
    const uint32_t m = (uint32_t)(((uint64_t)n + stride - 1) / stride);
    if (!c->view_stream) {
        SPHX_HIP(c, hipStreamCreateWithFlags(&c->view_stream, hipStreamNonBlocking));
        SPHX_HIP(c, hipEventCreateWithFlags(&c->view_packed, hipEventDisableTiming));
        SPHX_HIP(c, hipEventCreateWithFlags(&c->view_done, hipEventDisableTiming));
    } else {
        SPHX_HIP(c, hipEventSynchronize(c->view_done));  // the previous transfer still owns the buffers
    }
    if (m > c->view_cap) {
        if (c->view_dev) hipFree(c->view_dev);
        if (c->view_host) hipHostFree(c->view_host);
        c->view_dev = nullptr;
        c->view_host = nullptr;
        c->view_cap = 0;
        SPHX_HIP(c, hipMalloc((void**)&c->view_dev, (size_t)m * 12));
        SPHX_HIP(c, hipHostMalloc((void**)&c->view_host, (size_t)m * 12, hipHostMallocDefault));
        c->view_cap = m;
    }
    if (m) {
        hipLaunchKernelGGL(k_view_pack, dim3(nblocks(m)), dim3(256), 0, c->stream, c->pv(), n, stride, c->view_dev);
        SPHX_HIP(c, hipEventRecord(c->view_packed, c->stream));
        SPHX_HIP(c, hipStreamWaitEvent(c->view_stream, c->view_packed, 0));
        SPHX_HIP(c, hipMemcpyAsync(c->view_host, c->view_dev, (size_t)m * 12, hipMemcpyDeviceToHost, c->view_stream));
    }
    SPHX_HIP(c, hipEventRecord(c->view_done, c->view_stream));
    c->view_count = m;
    c->view_pending = true;
    if (out_count) *out_count = m;
    return SPHX_OK;
}

int sphx_view_fetch(sphx_ctx* c, int wait, const float** out_xys, uint32_t* out_count) {
    if (!c || !out_xys || !out_count) return SPHX_ERR_INVALID_ARGUMENT;
    if (!c->view_pending) return c->fail(SPHX_ERR_NOT_READY, "no sphx_view_request outstanding");
    SPHX_HIP(c, hipSetDevice(c->device));
    if (wait) {
        SPHX_HIP(c, hipEventSynchronize(c->view_done));
    } else if (hipEventQuery(c->view_done) != hipSuccess) {
        return SPHX_ERR_NOT_READY;  // not an error worth a message: poll again
    }
    *out_xys = c->view_host;
    *out_count = c->view_count;
    return SPHX_OK;
}

static int download_particles(sphx_ctx* c, float* pos_xy, float* vel_xy, float* density, uint32_t* particle_id) {
    SPHX_HIP(c, hipSetDevice(c->device));
    flush_pending_advect(c);
    const size_t n = c->N;
    if (n) {
        if (pos_xy) SPHX_HIP(c, hipMemcpyAsync(pos_xy, c->posA, n * 8, hipMemcpyDeviceToHost, c->stream));
        if (vel_xy) SPHX_HIP(c, hipMemcpyAsync(vel_xy, c->vel, n * 8, hipMemcpyDeviceToHost, c->stream));
        if (density) SPHX_HIP(c, hipMemcpyAsync(density, c->density, n * 4, hipMemcpyDeviceToHost, c->stream));
        if (particle_id) SPHX_HIP(c, hipMemcpyAsync(particle_id, c->pid, n * 4, hipMemcpyDeviceToHost, c->stream));
    }
    SPHX_HIP(c, hipStreamSynchronize(c->stream));
    return SPHX_OK;
}

int sphx_download(sphx_ctx* c, float* pos_xy, float* vel_xy, float* density, uint32_t* particle_id) {
    if (!c) return SPHX_ERR_INVALID_ARGUMENT;
    if (c->in_step) return c->fail(SPHX_ERR_NOT_READY, "sphx_download between step_begin and step_finish");
    return download_particles(c, pos_xy, vel_xy, density, particle_id);
}

// (between the two phases of a WCSPH step nothing is queued: sphx_wcsph_step_begin has waited for its last kernel, and
// sphx_wcsph_step_finish changes the velocities alone)
int sphx_debug_download_wcsph_half_step(sphx_ctx* c, float* pos_xy, float* vel_xy, float* density, uint32_t* particle_id) {
    if (!c) return SPHX_ERR_INVALID_ARGUMENT;
    if (!c->in_step || !c->in_wcsph)
        return c->fail(SPHX_ERR_NOT_READY, "sphx_debug_download_wcsph_half_step outside sphx_wcsph_step_begin .. sphx_wcsph_step_finish");
    return download_particles(c, pos_xy, vel_xy, density, particle_id);
}

int sphx_download_boundary(sphx_ctx* c, float* xy, uint32_t* boundary_id) {
    if (!c) return SPHX_ERR_INVALID_ARGUMENT;
    SPHX_HIP(c, hipSetDevice(c->device));
    const size_t n = c->B;
    if (n) {
        if (xy) SPHX_HIP(c, hipMemcpyAsync(xy, c->bpos, n * 8, hipMemcpyDeviceToHost, c->stream));
        if (boundary_id) SPHX_HIP(c, hipMemcpyAsync(boundary_id, c->bid, n * 4, hipMemcpyDeviceToHost, c->stream));
    }
    SPHX_HIP(c, hipStreamSynchronize(c->stream));
    return SPHX_OK;
}

int sphx_download_solver_state(sphx_ctx* c, float* alpha, float* kappa, float* stiffness) {
    if (!c) return SPHX_ERR_INVALID_ARGUMENT;
    SPHX_HIP(c, hipSetDevice(c->device));
    const size_t n = c->N;
    if (n) {
        if (alpha) SPHX_HIP(c, hipMemcpyAsync(alpha, c->alpha, n * 4, hipMemcpyDeviceToHost, c->stream));
        if (kappa) SPHX_HIP(c, hipMemcpyAsync(kappa, c->kappa, n * 4, hipMemcpyDeviceToHost, c->stream));
        if (stiffness) SPHX_HIP(c, hipMemcpyAsync(stiffness, c->stiff, n * 4, hipMemcpyDeviceToHost, c->stream));
    }
    SPHX_HIP(c, hipStreamSynchronize(c->stream));
    return SPHX_OK;
}

int sphx_download_neighbors(sphx_ctx* c, uint16_t* counts, uint32_t* lists, uint64_t* out_total) {
    if (!c) return SPHX_ERR_INVALID_ARGUMENT;
    SPHX_HIP(c, hipSetDevice(c->device));
    const uint32_t n = c->N;
    if (out_total) *out_total = 0;
    if (!n) return SPHX_OK;
    // canonical export: counts (u16 pairs), start = exclusive prefix of count_total (host), lists concatenated
    DevTemp<uint16_t> d_counts;
    DevTemp<uint32_t> d_tot, d_start, d_out;
    SPHX_HIP(c, d_counts.alloc((size_t)n * 2));
    SPHX_HIP(c, d_tot.alloc(n));
    hipLaunchKernelGGL(k_export_counts, dim3(nblocks(n)), dim3(256), 0, c->stream, (const uint16_t*)c->nb_counts, n, (uint16_t*)d_counts, (uint32_t*)d_tot);
    std::vector<uint32_t> tot(n), start(n);
    SPHX_HIP(c, hipMemcpyAsync(tot.data(), d_tot, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    if (counts) SPHX_HIP(c, hipMemcpyAsync(counts, d_counts, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    SPHX_HIP(c, hipStreamSynchronize(c->stream));
    uint64_t total = 0;
    for (uint32_t i = 0; i < n; ++i) {
        start[i] = (uint32_t)total;
        total += tot[i];
    }
    if (out_total) *out_total = total;
    if (lists && total) {
        if (total > 0xFFFFFFFFull) return c->fail(SPHX_ERR_CAPACITY, "neighbour export larger than 2^32 entries");
        SPHX_HIP(c, d_start.alloc(n));
        SPHX_HIP(c, d_out.alloc(total));
        SPHX_HIP(c, hipMemcpyAsync(d_start, start.data(), (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(k_export_lists, dim3(nblocks(n)), dim3(256), 0, c->stream, c->nbv(), c->soff(), (const uint32_t*)d_start, n, (uint32_t*)d_out);
        SPHX_HIP(c, hipMemcpyAsync(lists, d_out, (size_t)total * 4, hipMemcpyDeviceToHost, c->stream));
        SPHX_HIP(c, hipStreamSynchronize(c->stream));
    }
    return SPHX_OK;
}

int sphx_download_cells(sphx_ctx* c, int which, uint32_t* first_particle, uint32_t* cidx, uint32_t* out_count) {
    if (!c || !out_count) return SPHX_ERR_INVALID_ARGUMENT;
    SPHX_HIP(c, hipSetDevice(c->device));
    // a4 (neighborhood_search.rs:142-165) is a run-length encoding of the sorted particles' cell codes: do exactly that.
    const uint32_t n = which ? c->B : c->N;
    const float2* p = which ? c->bpos : c->posA;
    std::vector<uint32_t> keys(n);
    if (n) {
        DevTemp<uint32_t> d_keys;
        SPHX_HIP(c, d_keys.alloc(n));
        hipLaunchKernelGGL(k_keys_of, dim3(nblocks(n)), dim3(256), 0, c->stream, p, n, c->K, (uint32_t*)d_keys);
        SPHX_HIP(c, hipMemcpyAsync(keys.data(), d_keys, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
        SPHX_HIP(c, hipStreamSynchronize(c->stream));
    }
    uint32_t m = 0;
    for (uint32_t i = 0; i < n; ++i) {
        if (i == 0 || keys[i] != keys[i - 1]) {
            if (first_particle && cidx) {
                first_particle[m] = i;
                cidx[m] = keys[i];
            }
            ++m;
        }
    }
    if (first_particle && cidx) {
        first_particle[m] = n;
        cidx[m] = 0xFFFFFFFFu;
    }
    *out_count = m + 1;
    return SPHX_OK;
}

uint32_t sphx_last_flags(const sphx_ctx* c) { return c ? c->step_flags : 0u; }

int sphx_grid_info(const sphx_ctx* c, int which, uint32_t* out4) {
    if (!c || !out4 || (which != 0 && which != 1)) return SPHX_ERR_INVALID_ARGUMENT;
    const Grid& g = which ? c->gstat : c->gdyn;
    out4[0] = g.nblk;
    out4[1] = g.len();
    out4[2] = g.nbx;
    out4[3] = g.nby;
    return SPHX_OK;
}

int sphx_get_viscosity(const sphx_ctx* c, uint32_t* model, float* fluid_viscosity, float* normalizer_laplacian) {
    if (!c) return SPHX_ERR_INVALID_ARGUMENT;
    if (model) *model = c->VK.visc_model;
    if (fluid_viscosity) *fluid_viscosity = c->VK.mu;
    if (normalizer_laplacian) *normalizer_laplacian = c->VK.vis_nlap;
    return SPHX_OK;
}

int sphx_get_constants(const sphx_ctx* c, float* o) {
    if (!c || !o) return SPHX_ERR_INVALID_ARGUMENT;
    o[0] = c->K.w_hinv;
    o[1] = c->K.w_norm;
    o[2] = c->K.w_ngrad;
    o[3] = c->K.p6_hsq;
    o[4] = c->K.p6_norm;
    o[5] = c->K.p6_ngrad;
    return SPHX_OK;
}


/* ---- multi-GPU tiles + sub-step entry points (include/sphx.h, "spatial tiles") ------------------------------------------ */
int sphx_reserve(sphx_ctx* c, uint32_t capacity) {
    if (!c) return SPHX_ERR_INVALID_ARGUMENT;
    c->ahead.valid = false;
    if (c->in_step) return c->fail(SPHX_ERR_NOT_READY, "sphx_reserve inside a step");
    SPHX_HIP(c, hipSetDevice(c->device));
    SPHX_HIP(c, hipStreamSynchronize(c->stream));
    if (c->N) return c->fail(SPHX_ERR_NOT_READY, "sphx_reserve must precede the upload");
    int rc = alloc_particles(c, capacity);
    if (rc) return rc;
    return ensure_index_scratch(c);
}

// General tiling: this context owns the cell rectangle `own`; `peers` are the rectangles of the tiles that touch it (edge or
// corner neighbours, at most 8), in the order the caller will pass the send / receive buffers.
int sphx_tile_configure_rect(sphx_ctx* c, const sphx_tile_rect* own, uint32_t halo_cells, const sphx_tile_rect* peers, uint32_t n_peers) {
    if (!c || !own || halo_cells == 0 || n_peers > MAX_TILE_PEERS || (n_peers && !peers)) return SPHX_ERR_INVALID_ARGUMENT;
    c->pending.bar_take_over();
    c->ahead.valid = false;
    auto bad = [](const sphx_tile_rect& r) { return r.x0 >= r.x1 || r.y0 >= r.y1 || r.x1 > 65536 || r.y1 > 65536; };
    if (bad(*own)) return c->fail(SPHX_ERR_INVALID_ARGUMENT, "tile rectangle must be non-empty and inside the u16 cell range");
    // a tile narrower than two halo widths would need ghosts from beyond its direct neighbours (edge tiles may be as narrow as
    // the fluid inside them: their outer side has no neighbour)
    for (uint32_t k = 0; k < n_peers; ++k)
        if (bad(peers[k])) return c->fail(SPHX_ERR_INVALID_ARGUMENT, "peer rectangle must be non-empty and inside the u16 cell range");
    if ((own->x0 > 0 && own->x1 < 65536 && own->x1 - own->x0 < 2 * halo_cells) || (own->y0 > 0 && own->y1 < 65536 && own->y1 - own->y0 < 2 * halo_cells))
        return c->fail(SPHX_ERR_INVALID_ARGUMENT, "a tile must be at least two halo widths wide");
    c->K.tile = TileRect{own->x0, own->x1, own->y0, own->y1};
    c->tile_halo = halo_cells;
    c->tile_npeers = n_peers;
    for (uint32_t k = 0; k < n_peers; ++k) c->tile_peer[k] = TileRect{peers[k].x0, peers[k].x1, peers[k].y0, peers[k].y1};
    c->tile_mode = true;
    return SPHX_OK;
}

// Strips along one axis (the 8-GPU layout): peers = {left, right} as far as they exist, in that order.
int sphx_tile_configure(sphx_ctx* c, int axis, uint32_t cell_lo, uint32_t cell_hi, uint32_t halo_cells, int has_left, int has_right) {
    if (!c || (axis != 0 && axis != 1) || cell_lo >= cell_hi || cell_hi > 65536 || halo_cells == 0) return SPHX_ERR_INVALID_ARGUMENT;
    c->ahead.valid = false;
    if (cell_hi - cell_lo < 2 * halo_cells) return c->fail(SPHX_ERR_INVALID_ARGUMENT, "a tile must be at least two halo widths wide");
    auto strip = [&](uint32_t lo, uint32_t hi) { return axis ? sphx_tile_rect{0u, 65536u, lo, hi} : sphx_tile_rect{lo, hi, 0u, 65536u}; };
    const sphx_tile_rect own = strip(cell_lo, cell_hi);
    sphx_tile_rect peers[2];
    uint32_t np = 0;
    if (has_left) peers[np++] = strip(0u, cell_lo);          // everything on the low side: only the part within the halo matters
    if (has_right) peers[np++] = strip(cell_hi, 65536u);
    c->tile_strip_left = has_left != 0;
    c->tile_strip_right = has_right != 0;
    int rc = sphx_tile_configure_rect(c, &own, halo_cells, peers, np);
    // the rectangle form rejects interior tiles only; strips keep the stricter historical check above
    return rc;
}

int sphx_tile_upload(sphx_ctx* c, const float* pos_xy, const float* vel_xy, const uint32_t* ids, uint32_t n) {
    if (!c || !c->tile_mode) return SPHX_ERR_INVALID_ARGUMENT;
    c->pending.bar_take_over();
    c->ahead.valid = false;
    int rc = sphx_upload(c, pos_xy, vel_xy, n);
    if (rc) return rc;
    if (n) {
        DevTemp<uint32_t> d_ids;
        if (ids) {
            SPHX_HIP(c, d_ids.alloc(n));
            SPHX_HIP(c, hipMemcpyAsync(d_ids, ids, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
        }
        hipLaunchKernelGGL(k_set_ids, dim3(nblocks(n)), dim3(256), 0, c->stream, c->pid, (const uint32_t*)d_ids.p, n, 0x80000000u);
        SPHX_HIP(c, hipStreamSynchronize(c->stream));
    }
    // per-workgroup send counts, and behind them one "sends anything" word per workgroup (TileClassArgs)
    if ((rc = dev_alloc(c, &c->tile_blk, (size_t)(nblocks(c->capN) + 8) * MAX_TILE_PEERS + nblocks(c->capN) + 8))) return rc;
    const uint32_t need = nblocks(c->capN, std::min(SCAN_TILE, SCAN1_TILE)) + 1;
    if (need > c->scan_partials_cap) {
        if ((rc = dev_alloc(c, &c->scan_partials, need))) return rc;
        c->scan_partials_cap = need;
    }
    c->cached_n = n;
    c->n_owned = n;
    return SPHX_OK;
}

// Fill the DEVICE send buffers ((1 + cap_records) * 32 bytes each; record 0 = header holding the count), one per configured peer,
// with the owned particles inside that peer's rectangle grown by the halo width, in ascending local order; retire what this tile no
// longer holds.
static int tile_pack_impl(sphx_ctx* c, float advect_dt, void* const* d_send, uint32_t n_send, uint32_t cap_records) {
    if (!c || !c->tile_mode || n_send != c->tile_npeers || (n_send && !d_send)) return SPHX_ERR_INVALID_ARGUMENT;
    lists_went_stale(c);  // (positions advance / retire here; the re-grid behind the exchange rebuilds the lists)
    SPHX_HIP(c, hipSetDevice(c->device));
    const uint32_t n = c->N;
    hipStream_t st = c->stream;
    TilePeers P{};
    P.n = n_send;
    for (uint32_t k = 0; k < n_send; ++k) {
        if (!d_send[k]) return SPHX_ERR_INVALID_ARGUMENT;
        P.rect[k] = c->tile_peer[k];
        P.out[k] = (HaloRec*)d_send[k];
    }
    if (!n) {
        for (uint32_t k = 0; k < n_send; ++k) SPHX_HIP(c, hipMemsetAsync(d_send[k], 0, 32, st));
        if (!c->external_stream) SPHX_HIP(c, hipStreamSynchronize(st));
        return SPHX_OK;
    }
    const uint32_t nb = nblocks(n);
    if (advect_dt > 0 && !(c->tile_pending_dt > 0.0f) && c->pending.take_over_class(n, advect_dt)) {
        // the loop's last density correction has counted the kept particles' cells and the records to send: the advection is left to
        // the re-grid's gather (as is the owner bit of particles that stay as ghosts), and only the workgroups that send anything are
        // visited again.  (Taken over: the pending advection and the owner fix below complete the count.)
        c->tile_band_packs += 1;
        c->tile_pending_dt = advect_dt;
        c->tile_pending_n = n;
        c->tile_fix_owner = true;
        if (n_send)
            launch(c, "tile_pack(band)", 0.0, [&] {
                hipLaunchKernelGGL(k_tile_offsets, dim3(1), dim3(1024), 0, st, c->tile_blk, nb, P);
                hipLaunchKernelGGL(k_tile_pack, dim3(nb), dim3(256), 0, st, (const float2*)c->vel, c->posA, c->pid, (const float*)c->kappa, (const float*)c->stiff, n,
                                   c->K, c->tile_halo, P, (const uint32_t*)c->tile_blk, cap_records, advect_dt, CountArgs{}, c->d_scal, 0u,
                                   (const uint32_t*)(c->tile_blk + (size_t)(nblocks(c->capN) + 8) * MAX_TILE_PEERS));
            });
        if (!c->external_stream) SPHX_HIP(c, hipStreamSynchronize(st));
        return SPHX_OK;
    }
    // the packing pass ends with the first pass of the re-grid that follows the exchange — cell and histogram of the particles the
    // tile keeps (build_grid then counts the arrivals only); not when the directory is about to change
    CountArgs ca{};
    flush_pending_advect(c);
    if (!c->no_fused_count && c->gdyn.len() && !c->boundary_changed && !c->need_expand && !c->need_recover && !c->recover_streak && !c->tails_dirty &&
        c->builds_since_cover + 1 < COVER_PERIOD) {
        drop_fused_count(c);
        ca = count_args(c, 0.0f);
        c->pending.made_by_pack(n);
    }
    // with the count fused in, nothing reads the kept particles' records before the re-grid's gather moves them: that gather applies
    // the advection (the same two operations) on the way, and this pass does not write the 24 bytes per particle
    const bool defer = advect_dt > 0 && ca.hist != nullptr && c->tile_defer_advect;
    if (defer) {
        c->tile_pending_dt = advect_dt;
        c->tile_pending_n = n;
    }
    launch(c, advect_dt > 0 ? "advect+tile_pack" : "tile_pack", (20.0 + 20.0 + 8.0 + ((advect_dt > 0 && !defer) ? 24.0 : 0.0) + (ca.hist ? 12.0 : 0.0)) * n, [&] {
        if (n_send) {
            hipLaunchKernelGGL(k_tile_count, dim3(nb), dim3(256), 0, st, c->pv(), (const uint32_t*)c->pid, n, c->K, c->tile_halo, P, c->tile_blk,
                               advect_dt);
            hipLaunchKernelGGL(k_tile_offsets, dim3(1), dim3(1024), 0, st, c->tile_blk, nb, P);
        }
        hipLaunchKernelGGL(k_tile_pack, dim3(nb), dim3(256), 0, st, (const float2*)c->vel, c->posA, c->pid, (const float*)c->kappa, (const float*)c->stiff, n, c->K,
                           c->tile_halo, P, (const uint32_t*)c->tile_blk, cap_records, advect_dt, ca, c->d_scal, defer ? 0u : 1u, (const uint32_t*)nullptr);
    });
    // the caller hands the buffers to the communication library next: on its own stream (sphx_set_stream) that is ordered by the
    // stream, otherwise the data has to be complete now
    if (!c->external_stream) SPHX_HIP(c, hipStreamSynchronize(st));
    return SPHX_OK;
}
int sphx_tile_pack_n(sphx_ctx* c, void* const* d_send, uint32_t n_send, uint32_t cap_records) { return tile_pack_impl(c, 0.0f, d_send, n_send, cap_records); }
// sphx_sub_advect + sphx_tile_pack_n in one pass over the particles (the packing kernels apply x += v* dt on the fly)
int sphx_tile_advect_pack_n(sphx_ctx* c, float dt, void* const* d_send, uint32_t n_send, uint32_t cap_records) {
    if (!(dt > 0) || !std::isfinite(dt)) return c ? c->fail(SPHX_ERR_INVALID_ARGUMENT, "dt must be positive and finite") : SPHX_ERR_INVALID_ARGUMENT;
    return tile_pack_impl(c, dt, d_send, n_send, cap_records);
}

// The record counts the packing pass wrote into the headers of the send buffers, on the host (round 6: the halo messages carry what
// was packed, not the buffers' capacity — the caller needs the counts before it can size its sends).
int sphx_tile_send_counts(sphx_ctx* c, void* const* d_send, uint32_t n_send, uint32_t cap_records, uint32_t* out_counts) {
    if (!c || !c->tile_mode || n_send != c->tile_npeers || (n_send && (!d_send || !out_counts))) return SPHX_ERR_INVALID_ARGUMENT;
    if (!n_send) return SPHX_OK;
    SPHX_HIP(c, hipSetDevice(c->device));
    uint32_t* const h = (uint32_t*)c->mbox->send_counts;  // pinned
    static_assert(offsetof(HaloRec, id) == 16, "header: the count sits in the id field");
    for (uint32_t k = 0; k < n_send; ++k) {
        if (!d_send[k]) return SPHX_ERR_INVALID_ARGUMENT;
        SPHX_HIP(c, hipMemcpyAsync(&h[k], (const char*)d_send[k] + 16, 4, hipMemcpyDeviceToHost, c->stream));
    }
    SPHX_HIP(c, hipStreamSynchronize(c->stream));
    for (uint32_t k = 0; k < n_send; ++k) out_counts[k] = std::min(h[k], cap_records);
    return SPHX_OK;
}

// Append the records received from the peers (d_recv[k] may be NULL) behind the particles sphx_tile_pack_n kept.  The local
// count becomes an upper bound until sphx_sub_regrid.
int sphx_tile_apply_n(sphx_ctx* c, const void* const* d_recv, uint32_t n_recv, uint32_t cap_records) {
    if (!c || !c->tile_mode || n_recv != c->tile_npeers || (n_recv && !d_recv)) return SPHX_ERR_INVALID_ARGUMENT;
    c->pending.bar_take_over();
    c->ahead.valid = false;
    SPHX_HIP(c, hipSetDevice(c->device));
    const uint32_t n = c->N;
    if ((uint64_t)n + (uint64_t)n_recv * cap_records > c->capN) return c->fail(SPHX_ERR_CAPACITY, "sphx_reserve a larger capacity: no room for the received halo");
    if (!n_recv) return SPHX_OK;
    hipStream_t st = c->stream;
    TileInbox B{};
    B.n = n_recv;
    for (uint32_t k = 0; k < n_recv; ++k) B.in[k] = (const HaloRec*)d_recv[k];
    launch(c, "tile_apply", (double)n_recv * cap_records * (32.0 + 40.0), [&] {
        hipLaunchKernelGGL(k_tile_apply, dim3(nblocks(n_recv * cap_records)), dim3(256), 0, st, B, cap_records, n, c->K, c->tile_halo, c->vel, c->posA,
                           c->pid, c->kappa, c->stiff, c->d_scal);
    });
    c->N = n + n_recv * cap_records;
    lists_went_stale(c);
    return SPHX_OK;
}

// Strip form (peers = left, right): buffers for a side that does not exist are ignored.
int sphx_tile_pack(sphx_ctx* c, void* d_left, void* d_right, uint32_t cap_records) {
    if (!c || !c->tile_mode || !d_left || !d_right) return SPHX_ERR_INVALID_ARGUMENT;
    void* bufs[2];
    uint32_t np = 0;
    if (c->tile_strip_left) bufs[np++] = d_left;
    if (c->tile_strip_right) bufs[np++] = d_right;
    SPHX_HIP(c, hipSetDevice(c->device));
    if (!c->tile_strip_left) SPHX_HIP(c, hipMemsetAsync(d_left, 0, 32, c->stream));
    if (!c->tile_strip_right) SPHX_HIP(c, hipMemsetAsync(d_right, 0, 32, c->stream));
    return sphx_tile_pack_n(c, bufs, np, cap_records);
}
int sphx_tile_apply(sphx_ctx* c, const void* d_from_left, const void* d_from_right, uint32_t cap_records) {
    if (!c || !c->tile_mode) return SPHX_ERR_INVALID_ARGUMENT;
    const void* bufs[2];
    uint32_t np = 0;
    if (c->tile_strip_left) bufs[np++] = d_from_left;
    if (c->tile_strip_right) bufs[np++] = d_from_right;
    return sphx_tile_apply_n(c, bufs, np, cap_records);
}

// Cell count (a1 + the histogram of a2) of the particles the tile holds right now — called between sphx_tile_pack_n and
// sphx_tile_apply_n, i.e. while the halo records are in flight: sphx_sub_regrid then only counts the received ones.  A no-op when
// the cell directory is about to change (the re-grid counts everything itself then).
int sphx_tile_count_kept(sphx_ctx* c) {
    if (!c || !c->tile_mode) return SPHX_ERR_INVALID_ARGUMENT;
    c->pending.bar_take_over();
    c->ahead.valid = false;
    SPHX_HIP(c, hipSetDevice(c->device));
    const uint32_t n = c->N;
    if (!n || !c->gdyn.len() || c->boundary_changed || c->need_expand || c->need_recover || c->recover_streak || c->tails_dirty) return SPHX_OK;
    drop_class_count(c);
    if (c->pending.is_for(n)) return SPHX_OK;  // counted already by the packing pass; a deferred advection stays deferred
    flush_pending_advect(c);
    drop_fused_count(c);
    launch(c, "cell_count", (8.0 + 4 + 4) * n, [&] {
        hipLaunchKernelGGL(k_key_count<false>, dim3(std::max(1u, nblocks(n))), dim3(256), 0, c->stream, PVr{nullptr, nullptr}, (const float2*)c->posA, n, 0.0f,
                           c->K, c->gdyn.view(), c->gdyn.hist, c->key, 1u, c->d_scal, 0u);
    });
    c->pending.made_by_pack(n);
    return SPHX_OK;
}

// re-grid of the local set (owned + ghosts): sort, neighbour lists, densities, alpha factors (dfsph.rs:512-518)
static int sub_regrid_impl(sphx_ctx* c, uint32_t* out_n_local, bool fuse_div, bool fuse_warm = false) {
    if (!c || !c->tile_mode) return SPHX_ERR_INVALID_ARGUMENT;
    c->ahead.valid = false;
    SPHX_HIP(c, hipSetDevice(c->device));
    int rc = update_neighborhood(c, false, 0.0f, true, fuse_div && c->fuse_div, fuse_warm && c->fuse_div);
    if (rc) return rc;
    // the re-grid's own publish ran BEFORE its gather: the host's cumulative count is now exactly "everything before this gather"
    c->owned_base = c->owned_cum;
    c->owned_dirty = true;
    c->cached_n = c->N;
    c->tile_density_ready = true;  // (fuse: the build left density and alpha of these positions)
    if (out_n_local) *out_n_local = c->N;
    return SPHX_OK;
}

// The NEXT step's non-pressure pass (dfsph.rs:436-477, with dt_prev = the step that is being finished) rides behind the kernels of the
// next sphx_sub_iteration — the one the caller expects to be the last of the step: the pass and the publish of its maximum are on the
// stream before the host has even seen that iteration's residual, so the round trip of the maximum overlaps the round trip of the
// verdict.  If the loop goes on (or anything else touches the context first) the pass is stale and sphx_sub_nonpressure runs again.
int sphx_sub_run_ahead(sphx_ctx* c, float dt_prev_of_next_step) {
    if (!c || !(dt_prev_of_next_step > 0) || !std::isfinite(dt_prev_of_next_step)) return SPHX_ERR_INVALID_ARGUMENT;
    c->sub_ahead_dt = c->run_ahead ? dt_prev_of_next_step : 0.0f;
    return SPHX_OK;
}
// which warm-start arrays the next re-grids move with their particles (tile mode; default both).  The tile loop switches one off
// when the solver loop that would read it will not warm-start (dfsph.rs:199 / :354) and therefore zeroes it first.
// tile mode: sphx_tile_advect_pack_n may leave the advection of the particles the tile keeps to the re-grid that follows the
// exchange (sphx_ctx::tile_pending_dt).  For callers that run pack -> exchange -> apply -> re-grid back to back (the tile loop).
int sphx_tile_band_packs(const sphx_ctx* c, uint32_t* out) {
    if (!c || !out) return SPHX_ERR_INVALID_ARGUMENT;
    *out = c->tile_band_packs;
    return SPHX_OK;
}
int sphx_tile_defer_advect(sphx_ctx* c, int on) {
    if (!c) return SPHX_ERR_INVALID_ARGUMENT;
    if (!on) flush_pending_advect(c);
    c->tile_defer_advect = on != 0;
    return SPHX_OK;
}
int sphx_set_tiling_invariant(sphx_ctx* c, int on) {
    if (!c) return SPHX_ERR_INVALID_ARGUMENT;
    if (c->in_step) return c->fail(SPHX_ERR_NOT_READY, "sphx_set_tiling_invariant between step_begin and step_finish");
    c->tiling_invariant = on != 0;
    c->ahead.valid = false;
    return SPHX_OK;
}
int sphx_tile_carry_warmstart(sphx_ctx* c, int kappa, int stiffness) {
    if (!c) return SPHX_ERR_INVALID_ARGUMENT;
    c->tile_carry_kappa = kappa != 0;
    c->tile_carry_stiff = stiffness != 0;
    return SPHX_OK;
}

int sphx_sub_nonpressure(sphx_ctx* c, float dt_prev, float* out_vmax_sq) {
    if (!c || !out_vmax_sq) return SPHX_ERR_INVALID_ARGUMENT;
    const bool ahead_ok = c->ahead.queued && c->ahead.valid;
    sub_step_enter(c);
    SPHX_HIP(c, hipSetDevice(c->device));
    const uint32_t n = c->N;
    *out_vmax_sq = 0.0f;
    if (!n) return SPHX_OK;
    c->step_flags = 0;
    uint32_t dt_prev_bits;
    std::memcpy(&dt_prev_bits, &dt_prev, 4);
    uint32_t seq;
    if (ahead_ok && c->ahead.seq && c->ahead.n == n && c->ahead.dt_bits == dt_prev_bits) {
        // the pass (and the publish of its maximum) went onto the stream behind the previous step's last solver iteration
        // (sphx_sub_run_ahead) and nothing has touched the context since: its result is, or is about to be, in the mailbox
        seq = c->ahead.seq;
        c->ahead.queued = false;
    } else {
        seq = ++c->seq;
        const VmaxArgs va{1u, take_vmax_slot(c), c->mbox_dev, seq};
        enqueue_nonpressure(c, dt_prev, va.vslot);
        hipLaunchKernelGGL(k_publish_vmax, dim3(1), dim3(64), 0, c->stream, c->d_scal, va);
    }
    int rc = wait_mailbox(c, seq);
    if (rc) return rc;
    const uint32_t vbits = c->mbox->vmax_sq_bits;
    std::memcpy(out_vmax_sq, &vbits, 4);
    return SPHX_OK;
}

int sphx_sub_predict(sphx_ctx* c, float dt) {
    if (!c) return SPHX_ERR_INVALID_ARGUMENT;
    sub_step_enter(c);
    SPHX_HIP(c, hipSetDevice(c->device));
    const uint32_t n = c->N;
    if (n) launch_predict(c, "velocity_prediction", dt);
    return SPHX_OK;
}

int sphx_sub_warmstart(sphx_ctx* c, int divergence, float dt) {
    if (!c) return SPHX_ERR_INVALID_ARGUMENT;
    sub_step_enter(c);
    if (c->handoff.first_errors_pending()) return c->fail(SPHX_ERR_NOT_READY, "warm start after sphx_sub_regrid_div (that pass has zeroed the warm-start values)");
    if (c->handoff.take_warm())  // sphx_sub_regrid_warm: the neighbour build has applied the divergence loop's warm start
        return divergence ? SPHX_OK : c->fail(SPHX_ERR_NOT_READY, "sphx_sub_regrid_warm must be followed by the divergence loop");
    SPHX_HIP(c, hipSetDevice(c->device));
    const uint32_t n = c->N;
    if (!n) return SPHX_OK;
    launch_warmstart(c, divergence != 0, dt, nullptr, false);
    return SPHX_OK;
}

// one solver iteration = compute_density_error/change + correct_velocity (dfsph.rs:217-218 / :372-373); returns this tile's
// residual sum over OWNED particles and the owned count (the caller all-reduces both and applies dfsph.rs:221-236 / :376-391)
int sphx_sub_regrid(sphx_ctx* c, uint32_t* out_n_local) { return sub_regrid_impl(c, out_n_local, false); }
int sphx_sub_regrid_div(sphx_ctx* c, uint32_t* out_n_local) { return sub_regrid_impl(c, out_n_local, true); }
int sphx_sub_regrid_warm(sphx_ctx* c, uint32_t* out_n_local) { return sub_regrid_impl(c, out_n_local, false, true); }
static int sub_iteration_impl(sphx_ctx* c, int divergence, float dt, int first, double* out_err_sum, uint64_t* out_n_owned, bool with_predict);
int sphx_sub_iteration(sphx_ctx* c, int divergence, float dt, int first, double* out_err_sum, uint64_t* out_n_owned) {
    return sub_iteration_impl(c, divergence, dt, first, out_err_sum, out_n_owned, false);
}
// sphx_sub_predict + the first density iteration (no warm start in between, dfsph.rs:199) in one call: the iteration's
// compute_density_error does the prediction on the way (k_compute_error<false, true>), as in the single context's step
int sphx_sub_predict_iteration(sphx_ctx* c, float dt, double* out_err_sum, uint64_t* out_n_owned) {
    if (!c) return SPHX_ERR_INVALID_ARGUMENT;
    if (!(dt > 0) || !std::isfinite(dt)) return c->fail(SPHX_ERR_INVALID_ARGUMENT, "dt must be positive and finite");
    if (!c->fuse_predict) {
        const int rc = sphx_sub_predict(c, dt);
        return rc ? rc : sub_iteration_impl(c, 0, dt, 1, out_err_sum, out_n_owned, false);
    }
    return sub_iteration_impl(c, 0, dt, 1, out_err_sum, out_n_owned, true);
}
static int sub_iteration_impl(sphx_ctx* c, int divergence, float dt, int first, double* out_err_sum, uint64_t* out_n_owned, bool with_predict) {
    if (!c || !out_err_sum) return SPHX_ERR_INVALID_ARGUMENT;
    sub_step_enter(c);
    SPHX_HIP(c, hipSetDevice(c->device));
    const uint32_t n = c->N;
    *out_err_sum = 0.0;
    if (out_n_owned) *out_n_owned = 0;
    if (!n) {
        // A tile without a particle: its re-grid may still have launched a build — over the slots a halo exchange could have filled,
        // an upper bound — and left that build's hand-off behind; the sorted count then came back as zero.  Nobody will take it: drop
        // it here, or the warm start of a later loop finds a stale "first errors" and refuses (seen with fixed iteration counts on a
        // strip that holds walls and no fluid).
        c->handoff.clear();
        return SPHX_OK;
    }
    // what a re-grid left is for the first divergence iteration behind it (enqueue_iteration takes it), and for nobody else
    const bool refused = c->handoff.first_errors_pending() && !(divergence && first);  // sphx_sub_regrid_div has done a loop's first compute_density_change
    if (refused || !c->handoff.first_errors_pending()) c->handoff.clear();
    if (refused) {
        ++c->seq, ++c->res_seq;  // (the numbers this iteration would have published under stay taken)
        return c->fail(SPHX_ERR_NOT_READY, "sphx_sub_regrid_div must be followed by the first divergence iteration");
    }
    // (no dt_dev, no LoopArgs: the caller all-reduces the residual; no out_warm: the warm start is sphx_sub_warmstart)
    IterSpec s{divergence != 0, first != 0, dt};
    const PredArgs host_dt{};  // (va.enabled = 0: dt is the argument)
    if (with_predict) s.pred = &host_dt;
    // Tile path: whichever correction turns out to be the last one of the loop has the advected positions in registers — it does
    // the re-grid's cell count of the particles the tile keeps and the send counts of the halo exchange that follows (what
    // k_tile_count / k_tile_pack read every particle again for).  Every correction does; the next one wipes the count.
    if (!divergence && c->tile_mode && c->tile_fuse_class && c->tile_defer_advect && c->tile_blk && !c->no_fused_count && c->gdyn.len() &&
        !c->boundary_changed && !c->need_expand && !c->need_recover && !c->recover_streak && !c->tails_dirty && c->builds_since_cover + 1 < COVER_PERIOD) {
        s.drop_count = true;
        s.ca = count_args(c, dt);
        s.tc.pid = c->pid;
        s.tc.blk = c->tile_blk;
        s.tc.any = c->tile_blk + (size_t)(nblocks(c->capN) + 8) * MAX_TILE_PEERS;  // (behind the counts: tile_upload's allocation)
        s.tc.halo = c->tile_halo;
        s.tc.n = c->tile_npeers;
        for (uint32_t k = 0; k < c->tile_npeers; ++k) s.tc.rect[k] = c->tile_peer[k];
    }
    const uint32_t seq = enqueue_iteration(c, s);
    if (c->sub_ahead_dt > 0.0f) {
        const float dtn = c->sub_ahead_dt;
        c->sub_ahead_dt = 0.0f;
        enqueue_run_ahead(c, dtn, true);
    }
    int rc = wait_mailbox(c, seq);
    if (rc) return rc;
    *out_err_sum = c->mbox->err_sum;
    if (c->tile_mode && c->owned_dirty) {
        // first publish behind the re-grid's gather: owned particles counted by that gather = growth of the cumulative counter since
        // the re-grid started (the difference is taken explicitly so that a tile that owns nothing reads 0, not its previous count)
        c->owned_last = c->mbox->owned_cum - c->owned_base;
        c->owned_cum = c->mbox->owned_cum;
        c->owned_dirty = false;
    }
    if (c->tile_mode) c->n_owned = (uint32_t)c->owned_last;
    if (out_n_owned) *out_n_owned = c->tile_mode ? c->n_owned : n;
    return SPHX_OK;
}

int sphx_sub_advect(sphx_ctx* c, float dt) {
    if (!c) return SPHX_ERR_INVALID_ARGUMENT;
    sub_step_enter(c);
    SPHX_HIP(c, hipSetDevice(c->device));
    const uint32_t n = c->N;
    if (n) launch(c, "advect", 24.0 * n, [&] { hipLaunchKernelGGL(k_advect, dim3(nblocks(n)), dim3(256), 0, c->stream, c->posA, (const float2*)c->vel, n, dt); });
    lists_went_stale(c);
    return SPHX_OK;
}

int sphx_profile_enable(sphx_ctx* c, int on) {
    if (!c) return SPHX_ERR_INVALID_ARGUMENT;
    hipSetDevice(c->device);
    if (!on) prof_resolve(c);
    c->profiling = on != 0;
    return SPHX_OK;
}
// Time only the launches with this label (NULL or "" = all), and of those only every `every`-th: a pair of event records every few
// steps instead of ~25 per step is cheap enough to stay on during a timed region, which is how bench.py measures the dominant
// kernel live.
int sphx_profile_filter(sphx_ctx* c, const char* label, uint32_t every) {
    if (!c) return SPHX_ERR_INVALID_ARGUMENT;
    c->prof_filter = label ? label : "";
    c->prof_every = every ? every : 1;
    c->prof_counter = 0;
    return SPHX_OK;
}
int sphx_profile_reset(sphx_ctx* c) {
    if (!c) return SPHX_ERR_INVALID_ARGUMENT;
    hipSetDevice(c->device);
    prof_resolve(c);
    c->prof_totals.clear();
    return SPHX_OK;
}
int sphx_profile_event_overhead(sphx_ctx* c, double* out_ms) {
    if (!c || !out_ms) return SPHX_ERR_INVALID_ARGUMENT;
    SPHX_HIP(c, hipSetDevice(c->device));
    SPHX_HIP(c, hipStreamSynchronize(c->stream));
    constexpr int N = 64;
    hipEvent_t a[N], b[N];
    for (int k = 0; k < N; ++k) {
        a[k] = prof_event(c);
        b[k] = prof_event(c);
        hipEventRecord(a[k], c->stream);
        hipEventRecord(b[k], c->stream);
    }
    SPHX_HIP(c, hipStreamSynchronize(c->stream));
    double tot = 0;
    for (int k = 0; k < N; ++k) {
        float ms = 0;
        hipEventElapsedTime(&ms, a[k], b[k]);
        tot += ms;
        c->ev_pool.push_back(a[k]);
        c->ev_pool.push_back(b[k]);
    }
    *out_ms = tot / N;
    return SPHX_OK;
}
int sphx_profile_get(sphx_ctx* c, sphx_kernel_time* out, uint32_t* inout_n) {
    if (!c || !inout_n) return SPHX_ERR_INVALID_ARGUMENT;
    hipSetDevice(c->device);
    prof_resolve(c);
    uint32_t k = 0;
    for (auto& kv : c->prof_totals) {
        if (out && k < *inout_n) {
            std::memset(&out[k], 0, sizeof(out[k]));
            std::strncpy(out[k].name, kv.first.c_str(), sizeof(out[k].name) - 1);
            out[k].launches = kv.second.launches;
            out[k].total_ms = kv.second.ms;
            out[k].algorithmic_bytes = kv.second.bytes;
        }
        ++k;
    }
    *inout_n = k;
    return SPHX_OK;
}

}  // extern "C"
