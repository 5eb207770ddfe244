// sphx_tiles.cpp — the multi-GPU step loop INSIDE libsphx ("internally may drive 1-8 GPUs"; 8(e)).
//
// The reference's caller holds ONE Box<dyn Solver> and calls simulation_step(&mut world, &mut time_manager)
// (src/sph/solver/mod.rs:12-18, src/main.rs:279); it knows nothing about tiles.  sphx_multi is that one object: it cuts the
// domain into spatial tiles (strips along the longer side, or columns cut again across: DESIGN.md §7), owns one libsphx context
// per tile, and runs the sub-steps of dfsph.rs:414-525 on all of them with one halo exchange per step and three scalar
// reductions.  Two ways to hold the tiles:
//   * sphx_multi_create        all tiles in THIS process, one host thread and one HIP stream per tile, devices given as a list
//                              (what a Rust host gets: multi-GPU behind the unchanged Solver boundary); halo records move with
//                              hipMemcpyPeerAsync between the tiles' buffers, ordered by HIP events — no host synchronisation;
//   * sphx_multi_create_rank   ONE tile of a multi-process run (one process per GPU, the bench contract); the records travel as
//                              grouped ncclSend / ncclRecv on the tile's stream (RCCL over xGMI, loaded at run time: libsphx has
//                              no link dependency on it), the scalars through the shared-memory all-reduce of sphx_shm_*; or
//                              through a communicator supplied by the caller (sphx_comm_ops: the tests use torch.distributed/gloo).
// The step loop itself (ring budget of the ghost band, adaptive band, re-partitioning, extra exchanges for long solver loops) is the
// one of tests/tiles_reference.py, statement for statement — that Python driver stays as the reference implementation the tests
// run over the CPU oracle; the HIP tiles driven from here must match it bit for bit (tests/test_gpu_multi.py).
#define __HIP_PLATFORM_AMD__ 1
#include <hip/hip_runtime_api.h>

#include <dlfcn.h>

#include <algorithm>
#include <atomic>
#include <cerrno>
#include <cmath>
#include <condition_variable>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <limits>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <array>
#include <chrono>
#include <vector>

#include "../../include/sphx.h"
#include "sphx_contour_merge.hpp"
#include "sphx_gauge_merge.hpp"
#include "sphx_multi_edit.hpp"
#include "sphx_multi_state_format.hpp"
#include "sphx_query_merge.hpp"
#include "sphx_render_merge.hpp"
#include "sphx_render_window.hpp"
#include "sphx_sample_window.hpp"
#include "sphx_stats_merge.hpp"
#include "sphx_track_merge.hpp"
#include "sphx_track_set.hpp"

namespace {

constexpr double INF = std::numeric_limits<double>::infinity();
constexpr uint32_t HALO_RECORD = SPHX_HALO_RECORD_BYTES;

struct Rect {
    uint32_t x0, x1, y0, y1;
    bool operator!=(const Rect& o) const { return x0 != o.x0 || x1 != o.x1 || y0 != o.y0 || y1 != o.y1; }
};

// GridProperties::position_to_mortoncellpos (neighborhood_search.rs:52-58) along one axis: same f32 operations as the device
inline uint32_t cell_coord(float v, float grid_min, float cell_inv) {
    const float c = (v - grid_min) * cell_inv;
    if (!(c > 0.0f)) return 0;  // NaN -> 0 like Rust's saturating cast
    if (c >= 65535.0f) return 65535;
    return (uint32_t)c;
}
inline bool in_rect(uint32_t cx, uint32_t cy, const Rect& r, uint32_t halo = 0) {
    return cx + halo >= r.x0 && cx < r.x1 + halo && cy + halo >= r.y0 && cy < r.y1 + halo;
}
inline bool rects_touch(const Rect& a, const Rect& b, uint32_t halo) {  // b grown by `halo` overlaps a (symmetric)
    const int64_t gx0 = (int64_t)b.x0 - halo, gx1 = (int64_t)b.x1 + halo, gy0 = (int64_t)b.y0 - halo, gy1 = (int64_t)b.y1 + halo;
    return (int64_t)a.x0 < gx1 && gx0 < (int64_t)a.x1 && (int64_t)a.y0 < gy1 && gy0 < (int64_t)a.y1;
}

// cut positions (cell indices) at particle-count quantiles; cuts[0] = 0, cuts[world] = 65536, strictly increasing
std::vector<uint32_t> quantile_cuts(std::vector<uint32_t> coords, int world) {
    std::sort(coords.begin(), coords.end());
    std::vector<uint32_t> cuts(world + 1, 0);
    for (int r = 1; r < world; ++r) cuts[r] = coords.empty() ? 0u : coords[(coords.size() * (size_t)r) / (size_t)world];
    cuts[world] = 65536;
    for (int r = 1; r <= world; ++r) cuts[r] = std::max(cuts[r], cuts[r - 1] + 1);
    return cuts;
}

// Diffusive re-partition ("re-partition when max/mean load > ~1.1"): every interior cut moves towards the heavier
// of its two tiles by half their difference expressed in cell columns, at most max_shift cells, never below two halo widths per
// tile.  Pure function of rank-identical inputs.
std::vector<uint32_t> rebalance_cuts(const std::vector<uint32_t>& cuts, const std::vector<double>& counts, uint32_t halo, double columns, int max_shift,
                                     double threshold = 1.05) {
    const int W = (int)counts.size();
    double total = 0, mx = 0;
    for (double c : counts) {
        total += c;
        mx = std::max(mx, c);
    }
    const double mean = total / std::max(W, 1);
    if (W < 2 || mean <= 0 || mx <= threshold * mean) return cuts;
    std::vector<int64_t> nw(cuts.begin(), cuts.end());
    for (int r = 1; r < W; ++r) {
        const int64_t d = (int64_t)std::nearbyint((counts[r] - counts[r - 1]) * 0.5 / std::max(columns, 1.0));  // round half to even, like Python
        nw[r] = (int64_t)cuts[r] + std::max<int64_t>(-max_shift, std::min<int64_t>(max_shift, d));
    }
    const int64_t min_w = 2 * (int64_t)halo + 2;
    for (int r = 1; r < W; ++r) nw[r] = std::max(nw[r], r > 1 ? nw[r - 1] + min_w : nw[r]);
    for (int r = W - 1; r > 0; --r) nw[r] = std::min(nw[r], r < W - 1 ? nw[r + 1] - min_w : nw[r]);
    for (int r = 1; r < W; ++r)
        if (std::llabs(nw[r] - (int64_t)cuts[r]) > max_shift) return cuts;  // the width rule pushed a cut further than allowed: keep all
    return std::vector<uint32_t>(nw.begin(), nw.end());
}

struct Layout {
    // strips: nx or ny == 1; grid: nx columns cut at xcuts, each column cut again at its own ycuts[ix]; rank = ix * ny + iy
    int axis = -1;  // >= 0: strips along this axis (cuts in xcuts)
    int nx = 1, ny = 1;
    std::vector<uint32_t> xcuts;
    std::vector<std::vector<uint32_t>> ycuts;
    int world() const { return axis >= 0 ? (int)xcuts.size() - 1 : nx * ny; }
    std::vector<Rect> rects() const {
        std::vector<Rect> out;
        if (axis >= 0) {
            for (size_t r = 0; r + 1 < xcuts.size(); ++r)
                out.push_back(axis == 0 ? Rect{xcuts[r], xcuts[r + 1], 0u, 65536u} : Rect{0u, 65536u, xcuts[r], xcuts[r + 1]});
        } else {
            for (int ix = 0; ix < nx; ++ix)
                for (int iy = 0; iy < ny; ++iy) out.push_back(Rect{xcuts[ix], xcuts[ix + 1], ycuts[ix][iy], ycuts[ix][iy + 1]});
        }
        return out;
    }
    bool rebalance(const std::vector<double>& counts, uint32_t halo, const double columns[2], int max_shift) {
        if (axis >= 0) {
            auto nw = rebalance_cuts(xcuts, counts, halo, columns[axis], max_shift);
            const bool ch = nw != xcuts;
            xcuts = nw;
            return ch;
        }
        const auto before_x = xcuts;
        const auto before_y = ycuts;
        std::vector<double> col(nx, 0.0);
        for (int ix = 0; ix < nx; ++ix)
            for (int iy = 0; iy < ny; ++iy) col[ix] += counts[ix * ny + iy];
        xcuts = rebalance_cuts(xcuts, col, halo, columns[0], max_shift);
        for (int ix = 0; ix < nx; ++ix) {
            std::vector<double> c(counts.begin() + ix * ny, counts.begin() + (ix + 1) * ny);
            ycuts[ix] = rebalance_cuts(ycuts[ix], c, halo, columns[1] / nx, max_shift);  // a column holds 1/nx of the particles
        }
        return xcuts != before_x || ycuts != before_y;
    }
};

// ---- communication between the tiles -------------------------------------------------------------------------------------
struct Comm {
    int rank = 0, world = 1;
    virtual ~Comm() {}
    // send[k] -> peers[k] (sbytes[k] of it), recv[k] <- peers[k] (rbytes[k]); ordered on the tile's stream (no host synchronisation)
    virtual int exchange(const std::vector<int>& peers, const std::vector<void*>& send, const std::vector<void*>& recv, const std::vector<size_t>& sbytes,
                         const std::vector<size_t>& rbytes, hipStream_t st) = 0;
    virtual int allreduce(const double* in, int n, int op, double* out) = 0;  // op 0 sum, 1 max; same bits on every rank
    // every rank's 8 doubles to every rank (out: world * 8).  Default: one all-reduce per rank (sums of one value and zeros: exact).
    virtual int allgather8(const double* in, double* out) {
        for (int r = 0; r < world; ++r) {
            double v[8];
            for (int k = 0; k < 8; ++k) v[k] = r == rank ? in[k] : 0.0;
            const int rc = allreduce(v, 8, 0, out + (size_t)r * 8);
            if (rc) return rc;
        }
        return SPHX_OK;
    }
    // can this transport move fewer bytes than the buffers hold?  (the caller-supplied function table has ONE size for all peers)
    virtual bool sized_messages() const { return true; }
    virtual void abort() {}  // this tile has failed: the tiles waiting for it in an all-reduce are released (they fail too)
    // the run is poisoned (a queued receive may never complete): tear the transport down WITHOUT waiting for what is enqueued on it
    virtual void abandon() {}
    virtual const char* name() const = 0;
};

// caller-supplied function table (sphx_comm_ops): the tests run it over torch.distributed
struct CallbackComm : Comm {
    sphx_comm_ops ops;
    explicit CallbackComm(const sphx_comm_ops& o) : ops(o) {
        rank = o.rank;
        world = o.world;
    }
    int exchange(const std::vector<int>& peers, const std::vector<void*>& send, const std::vector<void*>& recv, const std::vector<size_t>& sbytes,
                 const std::vector<size_t>&, hipStream_t st) override {
        if (peers.empty()) return SPHX_OK;
        return ops.exchange(ops.user, peers.data(), (int)peers.size(), send.data(), recv.data(), sbytes[0], (void*)st);  // (all sizes are the capacity)
    }
    bool sized_messages() const override { return false; }
    int allreduce(const double* in, int n, int op, double* out) override { return ops.allreduce(ops.user, in, n, op, out); }
    void abort() override {
        if (ops.abort) ops.abort(ops.user);
    }
    const char* name() const override { return "caller-supplied communicator"; }
};

// One process per GPU on one node: halo records as grouped ncclSend/ncclRecv on the tile's stream (RCCL over xGMI — point-to-point
// links, and the exchange is point-to-point with the <= 8 spatial neighbours: no ring collective anywhere), scalars through POSIX
// shared memory (they already sit in host memory on every rank: ~1 us instead of a device round trip).
struct RcclComm : Comm {
    struct Uid {
        char b[128];
    };
    void* lib = nullptr;
    void* comm = nullptr;
    sphx_shm* shm = nullptr;
    int (*p_get_uid)(Uid*) = nullptr;
    int (*p_init)(void**, int, Uid, int) = nullptr;
    int (*p_destroy)(void*) = nullptr;
    int (*p_abort)(void*) = nullptr;
    bool abandoned = false;
    int (*p_send)(const void*, size_t, int, int, void*, hipStream_t) = nullptr;
    int (*p_recv)(void*, size_t, int, int, void*, hipStream_t) = nullptr;
    int (*p_gstart)() = nullptr;
    int (*p_gend)() = nullptr;
    const char* (*p_err)(int) = nullptr;
    std::string err;

    int open(const char* job, int rank_, int world_, int device) {
        rank = rank_;
        world = world_;
        shm = sphx_shm_open(job, rank, world);
        if (!shm) {
            err = "sphx_shm_open failed";
            return SPHX_ERR_HIP;
        }
        const char* always = std::getenv("SPHX_RCCL_ALWAYS");  // test aid: bring RCCL up even for a single rank
        if (world == 1 && !(always && always[0] == '1')) return SPHX_OK;  // nothing to exchange
        // Every step of the bring-up ends in a status round over the shared segment: a rank that cannot go on says so, and ALL ranks
        // return an error together — nobody is left inside ncclCommInitRank (or the first all-reduce) waiting for a rank that gave up.
        auto agree = [&](bool ok, const char* stage) -> bool {
            double in = ok ? 0.0 : 1.0, out = 0.0;
            if (sphx_shm_allreduce(shm, &in, 1, 0, &out) != SPHX_OK) {
                if (ok || err.empty()) err = std::string("a rank did not reach the status round after: ") + stage;
                return false;
            }
            if (out > 0.0) {
                if (ok) err = std::to_string((int)out) + " other rank(s) failed: " + stage;
                return false;
            }
            return true;
        };
        for (const char* n : {"librccl.so", "librccl.so.1"}) {
            lib = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
            if (lib) break;
        }
        bool ok = lib != nullptr;
        if (!lib) err = std::string("dlopen(librccl.so): ") + dlerror();
        if (ok) {
            p_get_uid = (int (*)(Uid*))dlsym(lib, "ncclGetUniqueId");
            p_init = (int (*)(void**, int, Uid, int))dlsym(lib, "ncclCommInitRank");
            p_destroy = (int (*)(void*))dlsym(lib, "ncclCommDestroy");
            p_abort = (int (*)(void*))dlsym(lib, "ncclCommAbort");
            p_send = (int (*)(const void*, size_t, int, int, void*, hipStream_t))dlsym(lib, "ncclSend");
            p_recv = (int (*)(void*, size_t, int, int, void*, hipStream_t))dlsym(lib, "ncclRecv");
            p_gstart = (int (*)())dlsym(lib, "ncclGroupStart");
            p_gend = (int (*)())dlsym(lib, "ncclGroupEnd");
            p_err = (const char* (*)(int))dlsym(lib, "ncclGetErrorString");
            if (!p_get_uid || !p_init || !p_send || !p_recv || !p_gstart || !p_gend) {
                err = "librccl.so lacks the ncclSend/ncclRecv entry points";
                ok = false;
            }
        }
        if (const char* f = std::getenv("SPHX_TEST_FAIL_RCCL_LOAD"))  // test aid: this rank pretends librccl is missing
            if (std::atoi(f) == rank) {
                err = "librccl.so: load failure injected by SPHX_TEST_FAIL_RCCL_LOAD";
                ok = false;
            }
        if (!agree(ok, "loading librccl.so")) return SPHX_ERR_HIP;
        Uid id;
        std::memset(&id, 0, sizeof(id));
        int rc = 0;
        if (rank == 0) rc = p_get_uid(&id);
        // rank 0's id reaches the others through the shared segment (16 doubles = 128 bytes, two all-reduce rounds of 8: every other
        // rank contributes zeros; the bit patterns are sums of one value and zeros, i.e. exact — NaN payloads are avoided by
        // sending the bytes as small integers)
        double in[8], out[8];
        for (int part = 0; part < 16 && !rc; ++part) {
            for (int k = 0; k < 8; ++k) in[k] = rank == 0 ? (double)(unsigned char)id.b[part * 8 + k] : 0.0;
            if (sphx_shm_allreduce(shm, in, 8, 0, out)) rc = -1;
            for (int k = 0; k < 8; ++k) id.b[part * 8 + k] = (char)(unsigned char)out[k];
        }
        ok = rc == 0;
        if (!ok) err = "ncclGetUniqueId / broadcast of the RCCL unique id failed";
        if (ok && hipSetDevice(device) != hipSuccess) {
            err = "hipSetDevice";
            ok = false;
        }
        if (!agree(ok, "unique id / device selection")) return SPHX_ERR_HIP;
        rc = p_init(&comm, world, id, rank);
        if (const char* f = std::getenv("SPHX_TEST_FAIL_RCCL_INIT"))  // test aid: this rank reports a failed ncclCommInitRank
            if (std::atoi(f) == rank && !rc) rc = 1;
        if (rc) {
            err = std::string("ncclCommInitRank: ") + (p_err ? p_err(rc) : "error");
            if (comm && p_destroy && rc == 1 && std::getenv("SPHX_TEST_FAIL_RCCL_INIT")) p_destroy(comm);
            comm = nullptr;
        }
        if (!agree(rc == 0, "ncclCommInitRank")) {
            if (comm && p_destroy) p_destroy(comm);
            comm = nullptr;
            return SPHX_ERR_HIP;
        }
        return SPHX_OK;
    }
    void abort() override { sphx_shm_abort(shm); }
    // ncclCommDestroy waits for the operations enqueued on the communicator — for the very receive a poisoned run will never see
    // completed (round-3 advisor finding).  ncclCommAbort does not wait; without it the communicator is leaked rather than joined.
    void abandon() override { abandoned = true; }
    ~RcclComm() override {
        if (comm && abandoned) {
            if (p_abort) p_abort(comm);
        } else if (comm && p_destroy) {
            p_destroy(comm);
        }
        if (shm) sphx_shm_close(shm);
    }
    int exchange(const std::vector<int>& peers, const std::vector<void*>& send, const std::vector<void*>& recv, const std::vector<size_t>& sbytes,
                 const std::vector<size_t>& rbytes, hipStream_t st) override {
        if (peers.empty()) return SPHX_OK;
        if (!comm) return SPHX_ERR_NOT_READY;
        int rc = p_gstart();
        for (size_t k = 0; k < peers.size() && !rc; ++k) {
            rc = p_send(send[k], sbytes[k], /*ncclUint8*/ 1, peers[k], comm, st);
            if (!rc) rc = p_recv(recv[k], rbytes[k], 1, peers[k], comm, st);
        }
        const int rc2 = p_gend();
        if (rc || rc2) {
            err = std::string("ncclSend/ncclRecv: ") + (p_err ? p_err(rc ? rc : rc2) : "error");
            return SPHX_ERR_HIP;
        }
        return SPHX_OK;
    }
    int allreduce(const double* in, int n, int op, double* out) override { return sphx_shm_allreduce(shm, in, n, op, out); }
    int allgather8(const double* in, double* out) override { return sphx_shm_allgather(shm, in, 8, out); }
    const char* name() const override { return "RCCL send/recv (halo records) + shared-memory all-reduce (scalars)"; }
};

// All tiles in one process: the drivers are threads; a tile copies its peers' send buffers into its own receive buffers
// (hipMemcpyPeerAsync on its stream, behind an event the sender recorded after packing).  The host threads only meet to hand the
// event and buffer handles over; no one waits for the GPU.
struct LocalShared {
    int world;
    std::mutex mu;
    std::condition_variable cv;
    int arrived = 0;
    uint64_t gen = 0;
    bool aborted = false;
    struct Slot {
        std::vector<int> peers;
        std::vector<void*> send;
        hipEvent_t packed = nullptr;   // recorded by the owner after its pack kernels
        hipEvent_t drained = nullptr;  // recorded by the owner after it has copied everything it receives
        int device = 0;
        double val[8];
    };
    std::vector<Slot> slot;
    explicit LocalShared(int w) : world(w), slot(w) {}
    bool barrier() {  // false: another tile failed
        std::unique_lock<std::mutex> lk(mu);
        if (aborted) return false;
        const uint64_t g = gen;
        if (++arrived == world) {
            arrived = 0;
            ++gen;
            cv.notify_all();
        } else {
            cv.wait(lk, [&] { return gen != g || aborted; });
        }
        return !aborted;
    }
    void abort() {
        std::lock_guard<std::mutex> lk(mu);
        aborted = true;
        cv.notify_all();
    }
};
struct LocalComm : Comm {
    std::shared_ptr<LocalShared> sh;
    int device;
    LocalComm(std::shared_ptr<LocalShared> s, int r, int dev) : sh(std::move(s)), device(dev) {
        rank = r;
        world = sh->world;
        sh->slot[r].device = dev;
        hipSetDevice(dev);
        hipEventCreateWithFlags(&sh->slot[r].packed, hipEventDisableTiming);
        hipEventCreateWithFlags(&sh->slot[r].drained, hipEventDisableTiming);
    }
    ~LocalComm() override {
        hipSetDevice(device);
        hipEventDestroy(sh->slot[rank].packed);
        hipEventDestroy(sh->slot[rank].drained);
    }
    int exchange(const std::vector<int>& peers, const std::vector<void*>& send, const std::vector<void*>& recv, const std::vector<size_t>&,
                 const std::vector<size_t>& rbytes, hipStream_t st) override {
        if (world == 1) return SPHX_OK;
        LocalShared::Slot& me = sh->slot[rank];
        me.peers = peers;
        me.send = send;
        if (hipEventRecord(me.packed, st) != hipSuccess) return SPHX_ERR_HIP;
        if (!sh->barrier()) return SPHX_ERR_NOT_READY;  // everybody's send buffers and `packed` events are published
        for (size_t k = 0; k < peers.size(); ++k) {
            LocalShared::Slot& p = sh->slot[peers[k]];
            void* src = nullptr;
            for (size_t j = 0; j < p.peers.size(); ++j)
                if (p.peers[j] == rank) src = p.send[j];
            if (!src) return SPHX_ERR_INVALID_ARGUMENT;
            if (hipStreamWaitEvent(st, p.packed, 0) != hipSuccess) return SPHX_ERR_HIP;
            if (hipMemcpyPeerAsync(recv[k], device, src, p.device, rbytes[k], st) != hipSuccess) return SPHX_ERR_HIP;
        }
        if (hipEventRecord(me.drained, st) != hipSuccess) return SPHX_ERR_HIP;
        if (!sh->barrier()) return SPHX_ERR_NOT_READY;  // everybody's copies are queued ...
        // ... and nobody's next pack may overwrite a send buffer before its readers have drained it
        for (int p : peers)
            if (hipStreamWaitEvent(st, sh->slot[p].drained, 0) != hipSuccess) return SPHX_ERR_HIP;
        return SPHX_OK;
    }
    int allreduce(const double* in, int n, int op, double* out) override {
        if (world == 1) {
            for (int k = 0; k < n; ++k) out[k] = in[k];
            return SPHX_OK;
        }
        for (int k = 0; k < n; ++k) sh->slot[rank].val[k] = in[k];
        if (!sh->barrier()) return SPHX_ERR_NOT_READY;
        for (int k = 0; k < n; ++k) {
            double acc = sh->slot[0].val[k];
            for (int r = 1; r < world; ++r) acc = op == 1 ? std::max(acc, sh->slot[r].val[k]) : acc + sh->slot[r].val[k];  // rank order: same bits everywhere
            out[k] = acc;
        }
        if (!sh->barrier()) return SPHX_ERR_NOT_READY;
        return SPHX_OK;
    }
    int allgather8(const double* in, double* out) override {
        if (world == 1) {
            for (int k = 0; k < 8; ++k) out[k] = in[k];
            return SPHX_OK;
        }
        for (int k = 0; k < 8; ++k) sh->slot[rank].val[k] = in[k];
        if (!sh->barrier()) return SPHX_ERR_NOT_READY;
        for (int r = 0; r < world; ++r)
            for (int k = 0; k < 8; ++k) out[(size_t)r * 8 + k] = sh->slot[r].val[k];
        if (!sh->barrier()) return SPHX_ERR_NOT_READY;
        return SPHX_OK;
    }
    void abort() override { sh->abort(); }
    const char* name() const override { return "in-process tiles (peer copies ordered by HIP events)"; }
};

// sphx_multi_probe_record: what the multi keeps of the recording (points and gauges are copied at the call; the tiles hold the frames).
// A tile installs the recording of the current epoch in front of the first frame it is asked for, so a recording made before the first
// upload — when the contexts are not tiles yet — works like any other.
struct MultiProbe {
    std::vector<float> points;
    std::vector<sphx_gauge> gauges;
    int kind = 0, field = 0;
    float iso = 0.0f;
    uint32_t max_frames = 0, every = 1;
    bool on = false;
    uint64_t epoch = 0;  // counts the sphx_multi_probe_record calls
};

// ---- one tile ---------------------------------------------------------------------------------------------------------------
struct TileDriver {
    sphx_ctx* ctx = nullptr;
    std::unique_ptr<Comm> comm;
    sphx_params P;
    sphx_multi_options O;
    Layout layout;
    int device = 0;
    hipStream_t stream = nullptr, comm_stream = nullptr;
    hipEvent_t ev_packed = nullptr, ev_exchanged = nullptr;
    std::string err;
    uint32_t halo_max = 16, halo_now = 16, min_halo = 6;
    std::vector<int> spent;
    uint32_t last_div_iters = 1, last_div_warm = 0;
    uint32_t num_density_iters = 1, num_divergence_iters = 0;  // dfsph.rs:51,55
    uint32_t cap = 0;
    uint64_t exchanges = 0, rebalances = 0, steps = 0;
    uint64_t halo_bytes_packed = 0, halo_bytes_sent = 0;  // to all peers together, over all exchanges
    double ownership_seconds = 0.0;  // set-up: cells, owner and send-band counts of the global scene (host threads)
    int exact_exchange = -1;  // SPHX_EXACT_EXCHANGE: 1 always, 0 never, -1 (default) when a message at capacity is >= EXACT_MIN_BYTES
    // where the record counts have to travel first (a host wait for the packing kernels + one meeting of the ranks, ~20 us) only
    // messages that are worth it do: at 1 M particles per tile a strip's message is 0.3 MB at capacity (2 us on a link), at the 16 M
    // per tile of configs[3] / [4] it is 11 MB
    static constexpr size_t EXACT_MIN_BYTES = 1u << 20;
    const uint32_t boundary_margin = 256;
    double valid = INF, kvalid = INF, avalid = INF;
    Rect rect{}, clip_rect{};
    std::vector<int> peers;
    std::vector<Rect> peer_rects;
    std::vector<std::pair<void*, void*>> bufs;  // per rank: {send, recv} device buffers (allocated on first use)
    double columns[2] = {1, 1};
    uint64_t n_owned_local = 0, n_owned_global = 0;
    uint32_t n_local = 0;
    std::vector<float> boundary;
    std::vector<uint32_t> bcx, bcy;
    std::vector<uint32_t> clip_map;  // clipped boundary index -> index in `boundary` (the caller's order), renewed by every clip_boundary()
    float grid_min[2], cell_inv;
    // step in flight
    float step_dt_prev = 0, step_vmax = 0;
    bool in_step = false;
    float pending_advect_dt = 0.0f;
    bool overlap = false;  // sphx_multi_options.overlap_exchange / SPHX_MULTI_OVERLAP=1: records on a second stream, interior work meanwhile
    bool run_ahead_ok = true;  // SPHX_RUN_AHEAD=0 switches the run-ahead over the step boundary off (A/B runs)
    sphx_stats_rec* stats_dev = nullptr;  // sphx_multi_fluid_stats: this tile's 1 + SPHX_STATS_MAX_RECTS records (device, allocated on first use)

    bool poisoned = false;  // a collective step failed half-way: receives that will never complete may sit on the stream
    int fail(int rc, const std::string& what) {
        err = what;
        if (ctx && rc != SPHX_OK) {
            const char* e = sphx_last_error(ctx);
            if (e && *e) err += std::string(": ") + e;
        }
        if (rc != SPHX_OK && comm && comm->world > 1) {
            // the other tiles are (or will be) waiting for this one in an all-reduce: release them — they fail with NOT_READY at
            // once instead of sitting out the time-out (or, over RCCL, a receive nobody will ever send)
            comm->abort();
            poisoned = true;
        }
        return rc;
    }
#define TCHK(expr)                                \
    do {                                          \
        const int rc__ = (expr);                  \
        if (rc__) return fail(rc__, #expr);       \
    } while (0)

    ~TileDriver() {
        if (ctx && poisoned && comm && comm->world > 1 && std::string(comm->name()).find("in-process") == std::string::npos) {
            // one process per tile and the run has failed: a queued receive may never complete — do not wait for the stream (the
            // context, its stream and the exchange buffers are deliberately left to process exit) and do not let the communicator
            // wait for it either; the process is about to report the error and exit
            comm->abandon();
            ctx = nullptr;
            return;
        }
        if (ctx) {
            hipSetDevice(device);
            sphx_synchronize(ctx);
            sphx_set_stream(ctx, nullptr);
            sphx_destroy(ctx);
        }
        for (auto& b : bufs) {
            if (b.first) hipFree(b.first);
            if (b.second) hipFree(b.second);
        }
        if (stats_dev) hipFree(stats_dev);
        if (comm_stream) hipStreamDestroy(comm_stream);
        if (ev_packed) hipEventDestroy(ev_packed);
        if (ev_exchanged) hipEventDestroy(ev_exchanged);
        if (stream) hipStreamDestroy(stream);
    }

    int init(const sphx_params& params, int dev, const sphx_multi_options& opt, std::unique_ptr<Comm> c) {
        P = params;
        P.device = dev;
        O = opt;
        device = dev;
        comm = std::move(c);
        overlap = O.overlap_exchange != 0;
        if (const char* e = std::getenv("SPHX_MULTI_OVERLAP")) overlap = e[0] == '1';
        if (const char* e = std::getenv("SPHX_EXACT_EXCHANGE")) exact_exchange = e[0] == '1' ? 1 : (e[0] == '0' ? 0 : -1);
        if (const char* e = std::getenv("SPHX_RUN_AHEAD")) run_ahead_ok = e[0] != '0';
        halo_max = O.halo_cells ? O.halo_cells : 16;
        min_halo = std::min<uint32_t>(6, halo_max);
        halo_now = halo_max;
        grid_min[0] = P.grid_min[0];
        grid_min[1] = P.grid_min[1];
        cell_inv = 1.0f / P.smoothing_length;
        int rc = sphx_create(&P, &ctx);
        if (rc) return fail(rc, sphx_last_error(nullptr));
        if (hipSetDevice(dev) != hipSuccess || hipStreamCreateWithFlags(&stream, hipStreamNonBlocking) != hipSuccess ||
            hipStreamCreateWithFlags(&comm_stream, hipStreamNonBlocking) != hipSuccess ||
            hipEventCreateWithFlags(&ev_packed, hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&ev_exchanged, hipEventDisableTiming) != hipSuccess)
            return fail(SPHX_ERR_HIP, "hipStreamCreate / hipEventCreate");
        // the tile's kernels and its communication share one stream: pack -> exchange -> unpack are ordered by the stream
        TCHK(sphx_set_stream(ctx, stream));
        // the kept particles' advection rides on the re-grid's gather (with the exchange on a second stream too: the cells of the kept
        // particles are counted by the density loop's last correction or by the packing pass, not from their records)
        TCHK(sphx_tile_defer_advect(ctx, 1));
        bufs.assign(comm->world, {nullptr, nullptr});
        return SPHX_OK;
    }

    // ---- geometry
    int place() {
        const auto rects = layout.rects();
        rect = rects[comm->rank];
        peers.clear();
        for (int k = 0; k < comm->world; ++k)
            if (k != comm->rank && rects_touch(rect, rects[k], halo_max)) peers.push_back(k);
        if (peers.size() > SPHX_MAX_TILE_PEERS) return fail(SPHX_ERR_INVALID_ARGUMENT, "a tile touches more than 8 others: tiles are too small for this halo");
        auto too_narrow = [&](const Rect& r) {
            return (r.x0 > 0 && r.x1 < 65536 && r.x1 - r.x0 < 2 * halo_max) || (r.y0 > 0 && r.y1 < 65536 && r.y1 - r.y0 < 2 * halo_max);
        };
        if (too_narrow(rect)) return fail(SPHX_ERR_INVALID_ARGUMENT, "tiles must be at least two halo widths wide");
        for (int k : peers)
            if (too_narrow(rects[k])) return fail(SPHX_ERR_INVALID_ARGUMENT, "tiles must be at least two halo widths wide");
        peer_rects.clear();
        for (int k : peers) peer_rects.push_back(rects[k]);
        return configure();
    }
    int configure() {
        sphx_tile_rect own{rect.x0, rect.x1, rect.y0, rect.y1};
        std::vector<sphx_tile_rect> pr;
        for (const Rect& r : peer_rects) pr.push_back(sphx_tile_rect{r.x0, r.x1, r.y0, r.y1});
        sphx_tile_rect dummy{0, 1, 0, 1};
        TCHK(sphx_tile_configure_rect(ctx, &own, halo_now, pr.empty() ? &dummy : pr.data(), (uint32_t)pr.size()));
        return SPHX_OK;
    }
    int clip_boundary() {
        const uint32_t m = halo_max + 2 + (O.rebalance_every ? boundary_margin : 0);
        clip_rect = rect;
        std::vector<float> keep;
        clip_map.clear();  // (sphx_multi_query_radius: a tile's boundary_id indexes the clipped set; this is the way back to the caller's order)
        for (size_t i = 0; i < bcx.size(); ++i)
            if (in_rect(bcx[i], bcy[i], rect, m)) {
                keep.push_back(boundary[2 * i]);
                keep.push_back(boundary[2 * i + 1]);
                clip_map.push_back((uint32_t)i);
            }
        TCHK(sphx_set_boundary(ctx, keep.empty() ? nullptr : keep.data(), (uint32_t)(keep.size() / 2)));
        return SPHX_OK;
    }
    int buffers(std::vector<void*>& send, std::vector<void*>& recv) {
        const size_t bytes = (size_t)(1 + cap) * HALO_RECORD;
        hipSetDevice(device);
        for (int k : peers) {
            if (!bufs[k].first) {
                if (hipMalloc(&bufs[k].first, bytes) != hipSuccess || hipMalloc(&bufs[k].second, bytes) != hipSuccess) return fail(SPHX_ERR_HIP, "hipMalloc (halo buffers)");
                hipMemsetAsync(bufs[k].first, 0, bytes, stream);
                hipMemsetAsync(bufs[k].second, 0, bytes, stream);
            }
            send.push_back(bufs[k].first);
            recv.push_back(bufs[k].second);
        }
        return SPHX_OK;
    }

    // ---- set-up: every rank is given the SAME global arrays (deterministic scene) and keeps its own cells
    // kap / stf (sphx_multi_state_load): the warm-start sums of the particles, installed with them; the caller then restores the counts
    int setup(const Layout& lay, const float* pos, const float* vel, const uint32_t* ids, uint32_t n, const float* bnd, uint32_t nb, const float* kap = nullptr,
              const float* stf = nullptr) {
        layout = lay;
        if (layout.world() != comm->world) return fail(SPHX_ERR_INVALID_ARGUMENT, "layout and communicator disagree about the number of tiles");
        // Every rank is handed the GLOBAL scene (128 M particles at configs[4]): cells, bounding box, owner and send-band counts of all of
        // them — O(n W) — run on up to 8 host threads over contiguous slices (round 6; one thread took ~7 s of the set-up at 128 M).
        // Slices are merged in slice order: `mine` stays ascending, the counts are sums — the result does not depend on the thread count.
        const auto t_own0 = std::chrono::steady_clock::now();
        std::vector<uint32_t> cx(n), cy(n);
        uint32_t x0 = 0xFFFFFFFFu, x1 = 0, y0 = 0xFFFFFFFFu, y1 = 0;
        const unsigned T = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>({8u, std::max(1u, std::thread::hardware_concurrency()), (uint64_t)n / 65536u + 1u}));
        auto slices = [&](auto&& body) {  // body(t, i0, i1)
            std::vector<std::thread> th;
            for (unsigned t = 1; t < T; ++t) th.emplace_back([&, t] { body(t, (uint32_t)((uint64_t)n * t / T), (uint32_t)((uint64_t)n * (t + 1) / T)); });
            body(0u, 0u, (uint32_t)((uint64_t)n / T));
            for (auto& x : th) x.join();
        };
        {
            std::vector<std::array<uint32_t, 4>> bb(T, std::array<uint32_t, 4>{0xFFFFFFFFu, 0u, 0xFFFFFFFFu, 0u});
            slices([&](unsigned t, uint32_t i0, uint32_t i1) {
                std::array<uint32_t, 4> b = bb[t];
                for (uint32_t i = i0; i < i1; ++i) {
                    cx[i] = cell_coord(pos[2 * (size_t)i], grid_min[0], cell_inv);
                    cy[i] = cell_coord(pos[2 * (size_t)i + 1], grid_min[1], cell_inv);
                    b[0] = std::min(b[0], cx[i]);
                    b[1] = std::max(b[1], cx[i]);
                    b[2] = std::min(b[2], cy[i]);
                    b[3] = std::max(b[3], cy[i]);
                }
                bb[t] = b;
            });
            for (const auto& b : bb) {
                x0 = std::min(x0, b[0]);
                x1 = std::max(x1, b[1]);
                y0 = std::min(y0, b[2]);
                y1 = std::max(y1, b[3]);
            }
        }
        int rc = place();
        if (rc) return rc;
        const auto rects = layout.rects();
        const int W = comm->world;
        std::vector<uint32_t> mine;
        std::vector<std::vector<uint32_t>> mine_t(T);
        if (O.cap_records) {
            cap = O.cap_records;
            slices([&](unsigned t, uint32_t i0, uint32_t i1) {
                for (uint32_t i = i0; i < i1; ++i)
                    if (in_rect(cx[i], cy[i], rect)) mine_t[t].push_back(i);
            });
        } else {
            // particles a tile has to send to one peer: estimate from the global scene, with head-room for compression waves
            std::vector<uint8_t> touch((size_t)W * W, 0);
            for (int a = 0; a < W; ++a)
                for (int b = 0; b < W; ++b) touch[(size_t)a * W + b] = a != b && rects_touch(rects[a], rects[b], halo_max);
            std::vector<std::vector<uint64_t>> cnt_t(T, std::vector<uint64_t>((size_t)W * W, 0));
            slices([&](unsigned t, uint32_t i0, uint32_t i1) {
                std::vector<uint64_t>& cnt = cnt_t[t];
                int last = 0;  // (neighbouring particles of the scene mostly share their owner: try that rectangle first)
                for (uint32_t i = i0; i < i1; ++i) {
                    int a = -1;
                    if (in_rect(cx[i], cy[i], rects[last])) {
                        a = last;
                    } else {
                        for (int r = 0; r < W; ++r)
                            if (in_rect(cx[i], cy[i], rects[r])) {
                                a = r;
                                break;
                            }
                    }
                    if (a < 0) continue;
                    last = a;
                    if (a == comm->rank) mine_t[t].push_back(i);
                    for (int b = 0; b < W; ++b)
                        if (touch[(size_t)a * W + b] && in_rect(cx[i], cy[i], rects[b], halo_max)) cnt[(size_t)a * W + b] += 1;
                }
            });
            uint64_t near = 0;
            for (size_t k = 0; k < (size_t)W * W; ++k) {
                uint64_t c = 0;
                for (unsigned t = 0; t < T; ++t) c += cnt_t[t][k];
                near = std::max(near, c);
            }
            cap = (uint32_t)std::max<uint64_t>(1024, (uint64_t)(near * 1.5) + 1024);
        }
        {
            size_t tot = 0;
            for (const auto& m : mine_t) tot += m.size();
            mine.reserve(tot);
            for (const auto& m : mine_t) mine.insert(mine.end(), m.begin(), m.end());
        }
        ownership_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_own0).count();
        const uint64_t n_own = mine.size();
        if (sphx_num_particles(ctx)) {
            // a fresh decomposition of an edited scene: the tile starts from an empty particle set (the slot-bound warm-start values of
            // the old decomposition mean nothing for the new one)
            TCHK(sphx_upload(ctx, nullptr, nullptr, 0));
            TCHK(sphx_clear_cached(ctx));
        }
        TCHK(sphx_reserve(ctx, (uint32_t)((uint64_t)(n_own * 1.25) + 2ull * std::max<size_t>(2, peers.size()) * cap + 4096)));
        auto span = [](uint32_t lo, uint32_t hi, uint32_t cnt) { return cnt ? std::max<uint32_t>(1, hi - lo + 1) : 1u; };
        columns[0] = (double)n / span(x0, x1, n);
        columns[1] = (double)n / span(y0, y1, n);
        n_owned_local = n_own;
        boundary.assign(bnd, bnd + 2 * (size_t)nb);
        bcx.resize(nb);
        bcy.resize(nb);
        for (uint32_t i = 0; i < nb; ++i) {
            bcx[i] = cell_coord(bnd[2 * i], grid_min[0], cell_inv);
            bcy[i] = cell_coord(bnd[2 * i + 1], grid_min[1], cell_inv);
        }
        if (nb) {
            rc = clip_boundary();
            if (rc) return rc;
        }
        std::vector<float> p(2 * n_own), v(2 * n_own, 0.0f);
        std::vector<uint32_t> id(n_own);
        for (uint64_t k = 0; k < n_own; ++k) {
            const uint32_t i = mine[k];
            p[2 * k] = pos[2 * i];
            p[2 * k + 1] = pos[2 * i + 1];
            if (vel) {
                v[2 * k] = vel[2 * i];
                v[2 * k + 1] = vel[2 * i + 1];
            }
            id[k] = ids ? ids[i] : i;
        }
        if (kap && stf) {
            std::vector<float> ka(n_own), sf(n_own);
            for (uint64_t k = 0; k < n_own; ++k) {
                ka[k] = kap[mine[k]];
                sf[k] = stf[mine[k]];
            }
            TCHK(sphx_tile_carry_warmstart(ctx, 1, 1));  // (the re-grid below moves them with their particles)
            TCHK(sphx_tile_upload_state(ctx, p.data(), v.data(), id.data(), ka.data(), sf.data(), (uint32_t)n_own));
        } else {
            TCHK(sphx_tile_upload(ctx, p.data(), v.data(), id.data(), (uint32_t)n_own));
        }
        n_owned_global = n;
        num_density_iters = 1;
        num_divergence_iters = 0;
        spent.clear();
        return refresh();  // initial ghosts + the warm-up block (dfsph.rs:419-428): re-grid, densities, alpha
    }

    // ---- halo
    uint32_t cap_now() const {
        if (halo_now >= halo_max) return cap;
        const uint64_t scaled = ((uint64_t)cap * (halo_now + 4) + (halo_max + 4) - 1) / (halo_max + 4);
        return (uint32_t)std::min<uint64_t>(cap, std::max<uint64_t>(1024, scaled));
    }
    // div_next: the divergence loop follows at once and starts without a warm start — the re-grid's neighbour build then also does that
    // loop's first compute_density_change (sphx_sub_regrid_div)
    // warm_next: ... and starts WITH one: the build applies it (sphx_sub_regrid_warm; loop()'s sphx_sub_warmstart call is then a no-op)
    int refresh(bool div_next = false, bool warm_next = false) {  // halo exchange (migration + fresh ghosts) followed by the re-grid of the local set
        std::vector<void*> send, recv;
        int rc = buffers(send, recv);
        if (rc) return rc;
        const uint32_t c = cap_now();
        const size_t bytes = (size_t)(1 + c) * HALO_RECORD;  // only the part the band in use can fill travels
        void* dummy = nullptr;
        if (pending_advect_dt > 0.0f) {  // the advection of dfsph.rs:499-510 rides on the packing pass
            TCHK(sphx_tile_advect_pack_n(ctx, pending_advect_dt, send.empty() ? &dummy : send.data(), (uint32_t)send.size(), c));
            pending_advect_dt = 0.0f;
        } else {
            TCHK(sphx_tile_pack_n(ctx, send.empty() ? &dummy : send.data(), (uint32_t)send.size(), c));
        }
        // overlap_exchange: the records travel on a stream of their own (behind the packing kernels, in front of the unpacking one);
        // meanwhile the tile's stream counts the cells of the particles it kept — the first pass of the re-grid — so the exchange
        // latency hides behind interior work.  Off by default: with all tiles on ONE GPU (the only hardware this was measured on) the
        // two cross-stream event hand-offs cost more than the overlapped 8 us of counting (0.47 vs 0.40 ms/step, 2 x 500 k particles);
        // whether it pays over xGMI has to be measured on a multi-GPU node.
        // Round 6: the messages carry what was PACKED.  The packing pass leaves each message's record count in its header on the device;
        // the host fetches the counts (sphx_tile_send_counts: it waits for the packing kernels), the ranks tell each other (one meeting
        // at the shared segment: every rank's <= 8 counts to every rank), and ncclSend / ncclRecv move (1 + records) * 32 bytes rounded
        // up to 64 KiB instead of the buffers' capacity (1.5 x the estimate of the set-up + 1 024 records).  Capacity buffers unchanged:
        // a count beyond the capacity is clamped on both sides, k_tile_apply raises DF_HALO_CAP as before.
        std::vector<size_t> sbytes(peers.size(), bytes), rbytes(peers.size(), bytes);
        const bool exact = !peers.empty() && comm->sized_messages() && (exact_exchange == 1 || (exact_exchange < 0 && bytes >= EXACT_MIN_BYTES));
        if (exact) {
            uint32_t cnt[SPHX_MAX_TILE_PEERS] = {0};
            TCHK(sphx_tile_send_counts(ctx, send.data(), (uint32_t)send.size(), c, cnt));
            double row[8] = {0}, all[8 * 64];
            if (comm->world > 64) return fail(SPHX_ERR_INVALID_ARGUMENT, "more than 64 tiles");
            for (size_t k = 0; k < peers.size(); ++k) row[k] = (double)cnt[k];
            rc = comm->allgather8(row, all);
            if (rc) return fail(rc, "halo exchange failed (record counts)");
            const auto rects = layout.rects();
            auto round64k = [&](uint64_t records) { return std::min<size_t>(bytes, (((size_t)(1 + records) * HALO_RECORD + 65535u) >> 16) << 16); };
            for (size_t k = 0; k < peers.size(); ++k) {
                // my place in peer p's list of peers: p built it the way place() builds mine (ascending ranks that touch its rectangle)
                const int p = peers[k];
                int idx = 0, mine = -1;
                for (int q = 0; q < comm->world; ++q)
                    if (q != p && rects_touch(rects[p], rects[q], halo_max)) {
                        if (q == comm->rank) mine = idx;
                        idx += 1;
                    }
                if (mine < 0 || mine >= 8) return fail(SPHX_ERR_INVALID_ARGUMENT, "halo exchange: the peer relation is not symmetric");
                sbytes[k] = round64k(cnt[k]);
                rbytes[k] = round64k((uint64_t)std::min<double>(all[(size_t)p * 8 + mine], (double)c));
                halo_bytes_packed += (uint64_t)(1 + cnt[k]) * HALO_RECORD;
                halo_bytes_sent += sbytes[k];
            }
        } else {
            halo_bytes_sent += (uint64_t)bytes * peers.size();  // (what was packed is not known to the host on this path)
        }
        if (!peers.empty() && !overlap) {
            rc = comm->exchange(peers, send, recv, sbytes, rbytes, stream);
            if (rc) return fail(rc, "halo exchange failed");
        } else if (!peers.empty()) {
            if (hipEventRecord(ev_packed, stream) != hipSuccess || hipStreamWaitEvent(comm_stream, ev_packed, 0) != hipSuccess) return fail(SPHX_ERR_HIP, "event (pack -> exchange)");
            rc = comm->exchange(peers, send, recv, sbytes, rbytes, comm_stream);
            if (rc) return fail(rc, "halo exchange failed");
            if (hipEventRecord(ev_exchanged, comm_stream) != hipSuccess) return fail(SPHX_ERR_HIP, "event (exchange -> unpack)");
            TCHK(sphx_tile_count_kept(ctx));
            if (hipStreamWaitEvent(stream, ev_exchanged, 0) != hipSuccess) return fail(SPHX_ERR_HIP, "event wait");
        }
        const void* cdummy = nullptr;
        TCHK(sphx_tile_apply_n(ctx, recv.empty() ? &cdummy : (const void* const*)recv.data(), (uint32_t)recv.size(), c));
        TCHK(warm_next ? sphx_sub_regrid_warm(ctx, &n_local) : div_next ? sphx_sub_regrid_div(ctx, &n_local) : sphx_sub_regrid(ctx, &n_local));
        exchanges += 1;
        const double full = comm->world == 1 ? INF : (double)halo_now;
        valid = kvalid = full;  // rings (cells from the owned region) in which v* / kappa are exact
        avalid = full - 1;      // ... density and alpha (one traversal after the exchange)
        return SPHX_OK;
    }
    int need(double after) {  // make sure the owned region stays exact after an operation that leaves `after` valid rings
        return after < 0 ? refresh() : SPHX_OK;
    }
    void adapt_halo(int used) {
        spent.push_back(used);
        if (spent.size() > 8) spent.erase(spent.begin());
        const int mx = *std::max_element(spent.begin(), spent.end());
        const uint32_t nw = (uint32_t)std::max<int>((int)min_halo, std::min<int>((int)halo_max, mx + 2));
        if (nw != halo_now) {
            halo_now = nw;
            configure();
        }
    }
    int rebalance() {
        std::vector<double> counts(comm->world, 0.0);
        for (int base = 0; base < comm->world; base += 8) {  // the shared-memory reduction carries 8 doubles per call
            const int m = std::min(8, comm->world - base);
            double in[8] = {0}, out[8];
            for (int k = 0; k < m; ++k) in[k] = base + k == comm->rank ? (double)n_owned_local : 0.0;
            TCHK(comm->allreduce(in, m, 0, out));
            for (int k = 0; k < m; ++k) counts[base + k] = out[k];
        }
        if (!layout.rebalance(counts, halo_max, columns, (int)std::max<uint32_t>(1, std::min(halo_max / 4, min_halo)))) return SPHX_OK;
        int rc = place();
        if (rc) return rc;
        auto far = [&](uint32_t a, uint32_t b) { return (a > b ? a - b : b - a) > boundary_margin / 2; };
        if (!boundary.empty() && (far(rect.x0, clip_rect.x0) || far(rect.x1, clip_rect.x1) || far(rect.y0, clip_rect.y0) || far(rect.y1, clip_rect.y1))) {
            rc = clip_boundary();
            if (rc) return rc;
        }
        rebalances += 1;
        return SPHX_OK;
    }

    // ---- one solver loop (dfsph.rs:195-247 / :346-402) with the residual all-reduced over the tiles
    // predict_first: the velocity prediction has NOT been launched — the first iteration does it on the way (sphx_sub_predict_iteration;
    // the caller has checked that neither a warm start nor a halo exchange comes in between)
    int loop(bool divergence, float dt, uint32_t* out_iters, float* out_avg, uint32_t* out_warm, uint32_t* flags, bool predict_first = false) {
        const uint32_t prev = divergence ? num_divergence_iters : num_density_iters;
        const uint32_t fixed = divergence ? P.fixed_divergence_iterations : P.fixed_density_iterations;
        const float tol = divergence ? P.max_divergence_error : P.max_avg_density_error;
        const uint32_t capit = divergence ? P.max_divergence_iterations : P.max_density_iterations;
        const float rho0 = P.fluid_density;
        uint32_t warm = 0;
        if (prev > 1) {  // dfsph.rs:199 / :354
            int rc = need(std::min(valid, kvalid - 1));
            if (rc) return rc;
            TCHK(sphx_sub_warmstart(ctx, divergence ? 1 : 0, dt));
            valid = std::min(valid, kvalid - 1);
            warm = 1;
        }
        uint32_t iters = 0;
        float avg = 0;
        for (;;) {
            int rc = need(std::min(valid - 2, avalid - 1));
            if (rc) return rc;
            const double kv = std::min(valid - 1, avalid);
            double s = 0;
            uint64_t owned = 0;
            // Run-ahead over the step boundary: if this is the iteration the divergence loop is expected to end with (the count of the
            // previous step), and the ghost band still has a ring for it, the NEXT step's non-pressure pass goes onto the stream behind
            // it — the GPU works on it while the residual makes its round trip through the hosts' all-reduce, and the maximum is in the
            // mailbox when the next step asks for it.  A loop that goes on invalidates the pass (it simply runs again).
            if (divergence && run_ahead_ok && iters + 1 == std::max<uint32_t>(1, fixed ? fixed : prev) &&
                std::min(avalid, std::min(valid - 2, avalid - 1)) - 1 >= 0)
                TCHK(sphx_sub_run_ahead(ctx, dt));
            if (predict_first && iters == 0)
                TCHK(sphx_sub_predict_iteration(ctx, dt, &s, &owned));
            else
                TCHK(sphx_sub_iteration(ctx, divergence ? 1 : 0, dt, iters == 0, &s, &owned));
            n_owned_local = owned;
            valid = std::min(valid - 2, avalid - 1);
            kvalid = kv;
            iters += 1;
            double in[2] = {s, (double)owned}, out[2];
            TCHK(comm->allreduce(in, 2, 0, out));
            n_owned_global = (uint64_t)out[1];
            avg = (float)out[0] / (float)out[1];             // dfsph.rs:221
            if (divergence) avg = avg / rho0;                // dfsph.rs:376-377
            if (!std::isfinite(avg)) return fail(SPHX_ERR_NONFINITE, "residual is not finite (dfsph.rs:223,378)");
            if (fixed) {
                if (iters >= fixed) break;
                continue;
            }
            const float rel = divergence ? avg : avg / rho0;  // dfsph.rs:222
            if (rel * dt < tol) break;                        // dfsph.rs:226 / :381
            if (iters > capit) {                              // dfsph.rs:236 / :391
                *flags |= divergence ? SPHX_FLAG_DIVERGENCE_ITER_CAP : SPHX_FLAG_DENSITY_ITER_CAP;
                break;
            }
        }
        if (divergence)
            num_divergence_iters = iters;
        else
            num_density_iters = iters;
        *out_iters = iters;
        *out_avg = avg;
        *out_warm = warm;
        return SPHX_OK;
    }

    // ---- Solver::simulation_step, two-phase like the single context (the caller's TimeManager sits in between, dfsph.rs:478-480)
    int step_begin(float dt_prev, float* out_vmax) {
        if (in_step) return fail(SPHX_ERR_NOT_READY, "sphx_multi_step_begin called twice");
        int rc = need(std::min(avalid, valid) - 1);
        if (rc) return rc;
        float vsq = 0;
        TCHK(sphx_sub_nonpressure(ctx, dt_prev, &vsq));  // dfsph.rs:436-477
        double in = vsq, out = 0;
        TCHK(comm->allreduce(&in, 1, 1, &out));
        const float vs = (float)out;
        if (!std::isfinite(vs)) return fail(SPHX_ERR_NONFINITE, "max velocity is not finite (timemanager.rs:264 would panic)");
        step_vmax = std::sqrt(vs);  // dfsph.rs:479
        step_dt_prev = dt_prev;
        *out_vmax = step_vmax;
        in_step = true;
        return SPHX_OK;
    }
    int step_finish(float dt, sphx_step_stats* st) {
        if (!in_step) return fail(SPHX_ERR_NOT_READY, "sphx_multi_step_finish without sphx_multi_step_begin");
        in_step = false;
        sphx_step_stats s;
        std::memset(&s, 0, sizeof(s));
        s.dt_prev = step_dt_prev;
        s.dt = dt;
        s.vmax = step_vmax;
        // dfsph.rs:484-492 — folded into the density loop's first iteration when that one follows at once: no warm start
        // (dfsph.rs:199) and rings left for it (no halo exchange first, which would have to carry the predicted velocities)
        const double valid_pred = std::min(avalid, valid) - 1;
        const bool predict_first = num_density_iters <= 1 && std::min(valid_pred - 2, avalid - 1) >= 0;
        if (!predict_first) TCHK(sphx_sub_predict(ctx, dt));
        valid = valid_pred;
        int rc = loop(false, dt, &s.density_iterations, &s.avg_density_error, &s.warmstart_density, &s.flags, predict_first);  // dfsph.rs:496
        if (rc) return rc;
        pending_advect_dt = dt;  // dfsph.rs:499-510 (ghosts move with their exact copies' v*): applied by the refresh() below
        steps += 1;
        if (O.rebalance_every && comm->world > 1 && steps % O.rebalance_every == 0) {
            rc = rebalance();
            if (rc) return rc;
        }
        if (!O.fixed_halo && comm->world > 1)
            // rings of the interval that ends here: divergence loop of the previous step, non-pressure pass, this density loop, and
            // the one-ring offset of density/alpha (computed one traversal after the exchange)
            adapt_halo((int)(last_div_warm + 2 * last_div_iters + 1 + s.warmstart_density + 2 * s.density_iterations + 1));
        // warm-start values only travel through this re-grid if a loop will read them before it zeroes them: kappa by the next step's
        // density loop iff this one took more than one iteration (dfsph.rs:199), the stiffness by the divergence loop that follows iff
        // the previous one did (dfsph.rs:354)
        TCHK(sphx_tile_carry_warmstart(ctx, num_density_iters > 1, num_divergence_iters > 1));
        rc = refresh(num_divergence_iters <= 1, num_divergence_iters > 1);  // migration + ghosts, dfsph.rs:512-518 (warm start ahead <=> dfsph.rs:354)
        TCHK(sphx_tile_carry_warmstart(ctx, 1, 1));  // (an extra exchange in the middle of a loop moves values that are in use)
        if (rc) return rc;
        rc = loop(true, dt, &s.divergence_iterations, &s.avg_divergence, &s.warmstart_divergence, &s.flags);  // dfsph.rs:521
        if (rc) return rc;
        last_div_iters = s.divergence_iterations;
        last_div_warm = s.warmstart_divergence;
        s.neighbor_entries = 0;
        // sphx_multi_stats_record: a frame of this tile's owned particles behind the step's kernels (a flag test without a recording)
        TCHK(sphx_tile_stats_frame(ctx, dt, (uint32_t)n_owned_global));
        // sphx_multi_track_record: a frame of the tracked ids this tile owns, likewise
        TCHK(sphx_tile_track_frame(ctx));
        // sphx_multi_probe_record: a frame of the gauges and probe points, likewise
        if (probe && probe->on) {
            rc = probe_frame(dt);
            if (rc) return rc;
        }
        if (st) *st = s;
        return SPHX_OK;
    }

    // sphx_multi_probe_*: the multi's recording and the epoch this tile has installed
    const MultiProbe* probe = nullptr;
    uint64_t probe_epoch = 0;
    int probe_install() {
        if (!probe || probe_epoch == probe->epoch) return SPHX_OK;
        const MultiProbe& q = *probe;
        const uint32_t mp = (uint32_t)(q.points.size() / 2), ng = (uint32_t)q.gauges.size();
        const int rc = sphx_tile_probe_record(ctx, mp ? q.points.data() : nullptr, mp, ng ? q.gauges.data() : nullptr, ng, q.kind, q.field, q.iso,
                                              q.on ? q.max_frames : 0u, q.every);
        if (rc) {
            err = std::string("sphx_tile_probe_record: ") + sphx_last_error(ctx);
            return rc;
        }
        probe_epoch = q.epoch;
        return SPHX_OK;
    }
    // One finished step.  A frame that is due reads ring-1 ghosts like a query: the band is made final first (sample_band(): with the
    // band spent, the exchange the next step owes runs now — every tile takes the same decision — and that step then finds a full
    // band), then the tile's passes go onto its stream.  Nothing is waited for.
    int probe_frame(float dt) {
        int rc = probe_install();
        if (rc) return rc;
        if (sphx_tile_probe_due(ctx) && (rc = sample_band())) return rc;
        TCHK(sphx_tile_probe_frame(ctx, dt, (uint32_t)n_owned_global));
        return SPHX_OK;
    }
    // sphx_multi_gauge_levels, first half: table, sample pass and reduce pass go onto the tile's stream; nothing is waited for
    int gauge_enqueue(const sphx_gauge* gauges, uint32_t n_gauges, int kind, int field, float iso) {
        const int rc = sphx_tile_gauge_levels(ctx, gauges, n_gauges, kind, field, iso);
        if (rc) err = std::string("sphx_tile_gauge_levels: ") + sphx_last_error(ctx);  // (an argument or state error of one call: nobody is waiting in an all-reduce)
        return rc;
    }
    // ... second half: the parts, the compact values and the host's intervals come back
    std::vector<float> gauge_values;
    std::vector<uint32_t> gauge_lo_count;
    int gauge_fetch(sphx_gauge_part* parts, uint32_t n_gauges, uint64_t total, bool values) {
        if (values && gauge_values.size() < total) gauge_values.resize(total);
        gauge_lo_count.resize(2 * (size_t)n_gauges);
        const int rc = sphx_tile_gauge_fetch(ctx, parts, values ? gauge_values.data() : nullptr, gauge_lo_count.data());
        if (rc) err = std::string("sphx_tile_gauge_fetch: ") + sphx_last_error(ctx);
        return rc;
    }

    // sphx_multi_fluid_stats, first half: this tile's records go onto its stream, into stats_dev; nothing is waited for
    int stats_enqueue(const sphx_rect* rects, uint32_t n_rects) {
        if (hipSetDevice(device) != hipSuccess) return fail(SPHX_ERR_HIP, "hipSetDevice");
        if (!stats_dev && hipMalloc((void**)&stats_dev, (size_t)(1 + SPHX_STATS_MAX_RECTS) * sizeof(sphx_stats_rec)) != hipSuccess)
            return fail(SPHX_ERR_HIP, "hipMalloc (statistics records)");
        const int rc = sphx_tile_fluid_stats(ctx, rects, n_rects, SPHX_STATS_DEVICE_POINTERS, stats_dev);
        if (rc) {  // (an argument or state error of one call: the run goes on, nobody is waiting in an all-reduce)
            err = std::string("sphx_tile_fluid_stats: ") + sphx_last_error(ctx);
            return rc;
        }
        return SPHX_OK;
    }
    // ... second half: the records come back
    int stats_fetch(uint32_t n_rects, sphx_stats_rec* out) {
        if (hipSetDevice(device) != hipSuccess || hipMemcpyAsync(out, stats_dev, (size_t)(1 + n_rects) * sizeof(sphx_stats_rec), hipMemcpyDeviceToHost, stream) != hipSuccess ||
            hipStreamSynchronize(stream) != hipSuccess)
            return fail(SPHX_ERR_HIP, "copying the statistics records back");
        return SPHX_OK;
    }

    // sphx_multi_render*, first half: this tile's layer goes onto its stream, into the context's render scratch — the pixels of its
    // window only (sphx_render_window.hpp); nothing is waited for
    uint32_t render_win[4] = {0, 0, 0, 0};  // pixel columns [0], [1]) and rows [2], [3]) of the layer in flight; all zero: nothing to fetch
    sphx_render_layer render_dev{nullptr, nullptr, nullptr};
    std::vector<uint32_t> render_key, render_owner, render_rgba;  // the window on the host (grown on demand)
    int render_enqueue(const sphx_render_view* view, bool rgba) {
        if (hipSetDevice(device) != hipSuccess) return fail(SPHX_ERR_HIP, "hipSetDevice");
        const int rc = sphx_tile_render_window(ctx, view, rgba ? 1u : 0u, render_win, &render_dev);
        if (rc) err = std::string("sphx_tile_render_window: ") + sphx_last_error(ctx);  // (an argument or state error of one call: nobody is waiting in an all-reduce)
        return rc;
    }
    size_t render_pixels() const { return (size_t)(render_win[1] - render_win[0]) * (render_win[3] - render_win[2]); }
    // ... second half: the window's pixels are queued for the host (render_wait() completes the copies)
    int render_fetch(bool rgba) {
        const size_t n = render_pixels();
        if (!n) return SPHX_OK;
        if (render_key.size() < n) render_key.resize(n), render_owner.resize(n);
        if (rgba && render_rgba.size() < n) render_rgba.resize(n);
        if (hipSetDevice(device) != hipSuccess || hipMemcpyAsync(render_key.data(), render_dev.key, n * 4, hipMemcpyDeviceToHost, stream) != hipSuccess ||
            hipMemcpyAsync(render_owner.data(), render_dev.owner, n * 4, hipMemcpyDeviceToHost, stream) != hipSuccess ||
            (rgba && hipMemcpyAsync(render_rgba.data(), render_dev.rgba, n * 4, hipMemcpyDeviceToHost, stream) != hipSuccess))
            return fail(SPHX_ERR_HIP, "copying a layer's window back");
        return SPHX_OK;
    }
    int render_wait() {
        if (!render_pixels()) return SPHX_OK;
        if (hipSetDevice(device) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess) return fail(SPHX_ERR_HIP, "waiting for a layer's window");
        return SPHX_OK;
    }

    // sphx_multi_state_*, first half: the pass over this tile's arrays goes onto its stream; nothing is waited for.  The warm-start
    // sections are canonical: zeros where the next loop will not warm-start (dfsph.rs:199 / :354)
    sphx_tile_state_out state_out{};
    uint64_t state_dig[7] = {0};
    uint32_t state_owned = 0;
    int state_enqueue() {
        const uint32_t flags = (num_density_iters <= 1 ? SPHX_TILE_STATE_ZERO_KAPPA : 0u) | (num_divergence_iters <= 1 ? SPHX_TILE_STATE_ZERO_STIFFNESS : 0u);
        const int rc = sphx_tile_state_pack(ctx, flags, &state_out, nullptr, nullptr);
        if (rc) err = std::string("sphx_tile_state_pack: ") + sphx_last_error(ctx);  // (a state error of one call: nobody is waiting in an all-reduce)
        return rc;
    }
    // ... second half: the digests and the owned count come back
    int state_fetch() {
        const int rc = sphx_tile_state_fetch(ctx, state_dig, &state_owned);
        if (rc) err = std::string("sphx_tile_state_fetch: ") + sphx_last_error(ctx);
        return rc;
    }
    // ... and `words` 32-bit words per particle of one section into host memory (queued; state_wait() completes them)
    int state_copy(const void* d_section, uint32_t words, void* host) {
        if (!state_owned) return SPHX_OK;
        if (hipSetDevice(device) != hipSuccess || hipMemcpyAsync(host, d_section, (size_t)state_owned * words * 4, hipMemcpyDeviceToHost, stream) != hipSuccess)
            return fail(SPHX_ERR_HIP, "copying a checkpoint section back");
        return SPHX_OK;
    }
    int state_wait() {
        if (hipSetDevice(device) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess) return fail(SPHX_ERR_HIP, "waiting for the checkpoint sections");
        return SPHX_OK;
    }

    // sphx_multi_remove, first half: the marking pass over this tile's records goes onto its stream; nothing is waited for
    int edit_remove_enqueue(const sphx_rect* rects, uint32_t n_rects, uint32_t flags) {
        const int rc = sphx_tile_remove_mark(ctx, rects, n_rects, flags);
        if (rc) err = std::string("sphx_tile_remove_mark: ") + sphx_last_error(ctx);  // (an argument or state error of one call: nobody is waiting in an all-reduce)
        return rc;
    }
    // ... second half: the number of owned records the pass retired comes back
    uint32_t edit_removed = 0;
    int edit_remove_fetch() {
        const int rc = sphx_tile_remove_fetch(ctx, &edit_removed);
        if (rc) err = std::string("sphx_tile_remove_fetch: ") + sphx_last_error(ctx);
        return rc;
    }
    // ... and, once the sum over ALL tiles is known to be positive (the same decision on every tile): the counts follow, and one halo
    // exchange + re-grid drops the retired records and the ghosts of those that other tiles retired
    int edit_remove_finish(uint64_t total) {
        n_owned_local -= std::min<uint64_t>(n_owned_local, edit_removed);
        n_owned_global -= std::min<uint64_t>(n_owned_global, total);
        return refresh();
    }
    // sphx_multi_append: the records this tile owns under the current layout go behind its local set; then the exchange + re-grid.
    // owner[k]: the tile of record k (sphx_multi_edit::route, the same on every tile)
    int edit_append(const float* pos, const float* vel, uint32_t n_new, uint32_t first_id, const std::vector<int>& owner) {
        std::vector<float> p, v;
        std::vector<uint32_t> id;
        for (uint32_t k = 0; k < n_new; ++k) {
            if (owner[k] != comm->rank) continue;
            p.push_back(pos[2 * (size_t)k]);
            p.push_back(pos[2 * (size_t)k + 1]);
            if (vel) {
                v.push_back(vel[2 * (size_t)k]);
                v.push_back(vel[2 * (size_t)k + 1]);
            }
            id.push_back(first_id + k);
        }
        const uint32_t routed = (uint32_t)id.size();
        // room for the local set, the routed records and what one exchange appends (sphx_tile_apply_n: cap_now() slots per peer)
        const uint64_t room = (uint64_t)sphx_num_particles(ctx) + routed + (uint64_t)peers.size() * cap;
        if (room >= (1ull << 28)) return fail(SPHX_ERR_CAPACITY, "sphx_multi_append: more than 2^28 slots in one tile: use more tiles");
        TCHK(sphx_tile_grow(ctx, (uint32_t)room));
        TCHK(sphx_tile_append(ctx, p.data(), vel ? v.data() : nullptr, id.data(), routed));
        n_owned_local += routed;
        n_owned_global += n_new;
        return refresh();
    }

    // sphx_multi_sample_*: a query reads position, velocity and density of ring-1 ghosts.  They are final iff valid >= 1 (velocities)
    // and avalid >= 1 (densities) — the test step_begin() makes before its non-pressure pass.  With a ring left nothing happens; with
    // the band spent the exchange + re-grid that step_begin() owes run now (pending_advect_dt is zero after a finished step: the
    // step's own refresh() has applied it), and step_begin() then finds a full band.
    int sample_band() { return need(std::min(avalid, valid) - 1); }
    // first half: this tile's passes go onto its stream, into the context's sample scratch; nothing is waited for
    int sample_points_enqueue(const float* xy, uint32_t n, int kind, uint32_t fields) {
        const int rc = sphx_tile_sample_points(ctx, xy, n, kind, fields);
        if (rc) err = std::string("sphx_tile_sample_points: ") + sphx_last_error(ctx);  // (an argument or state error of one call: nobody is waiting in an all-reduce)
        return rc;
    }
    // ... second half: the records of the points this tile answered come back
    int sample_points_fetch(uint32_t* records, uint32_t cap, uint32_t* out_n) {
        const int rc = sphx_tile_sample_points_fetch(ctx, records, cap, out_n);
        if (rc) err = std::string("sphx_tile_sample_points_fetch: ") + sphx_last_error(ctx);
        return rc;
    }
    uint32_t sample_win[4] = {0, 0, 0, 0};  // lattice columns [0], [1]) and rows [2], [3]) of the window in flight; all zero: nothing to fetch
    std::vector<uint32_t> sample_host;      // the window's arrays on the host (grown on demand)
    int sample_window_enqueue(float x0, float y0, float dx, float dy, uint32_t nx, uint32_t ny, int kind, uint32_t fields) {
        const int rc = sphx_tile_sample_window(ctx, x0, y0, dx, dy, nx, ny, kind, fields, sample_win);
        if (rc) err = std::string("sphx_tile_sample_window: ") + sphx_last_error(ctx);
        return rc;
    }
    size_t sample_window_points() const { return (size_t)(sample_win[1] - sample_win[0]) * (sample_win[3] - sample_win[2]); }
    // ... second half: the window-sized arrays come back, density | fraction | velocity | count in sample_host
    int sample_window_fetch(uint32_t fields, sphx_sample_out* win) {
        const size_t np = sample_window_points();
        *win = sphx_sample_out{nullptr, nullptr, nullptr, nullptr};
        if (!np) return SPHX_OK;
        const size_t words = np * ((fields & SPHX_SAMPLE_FIELD_DENSITY ? 1u : 0u) + (fields & SPHX_SAMPLE_FIELD_FRACTION ? 1u : 0u) +
                                   (fields & SPHX_SAMPLE_FIELD_VELOCITY ? 2u : 0u) + (fields & SPHX_SAMPLE_FIELD_COUNT ? 1u : 0u));
        if (sample_host.size() < words) sample_host.resize(words);
        uint32_t* p = sample_host.data();
        if (fields & SPHX_SAMPLE_FIELD_DENSITY) win->density = (float*)p, p += np;
        if (fields & SPHX_SAMPLE_FIELD_FRACTION) win->fraction = (float*)p, p += np;
        if (fields & SPHX_SAMPLE_FIELD_VELOCITY) win->velocity = (float*)p, p += 2 * np;
        if (fields & SPHX_SAMPLE_FIELD_COUNT) win->count = p;
        const int rc = sphx_tile_sample_window_fetch(ctx, win);
        if (rc) err = std::string("sphx_tile_sample_window_fetch: ") + sphx_last_error(ctx);
        return rc;
    }

    // sphx_multi_query_radius: a query reads positions and ids of ring-1 ghosts only, and those are exact after every exchange (they move
    // with the advection that rides on one, and none is pending where the call is allowed): no sample_band(), nothing is exchanged.
    // first half: upload, selection and the counting walk go onto the tile's stream
    int query_enqueue(const float* xy, uint32_t n, float radius, uint32_t flags, bool nearest) {
        const int rc = sphx_tile_query_radius(ctx, xy, n, radius, flags, nearest ? 1u : 0u);
        if (rc) err = std::string("sphx_tile_query_radius: ") + sphx_last_error(ctx);
        return rc;
    }
    // ... second half, step 1: the totals come back, the emitting walk goes onto the stream
    sphx_tile_query_part query_part{};
    std::vector<uint32_t> query_host;   // the part's arrays on the host (grown on demand, kept between calls)
    std::vector<uint64_t> query_host_off;
    int query_size(uint64_t cap_entries) {
        query_part = sphx_tile_query_part{};
        const int rc = sphx_tile_query_fetch(ctx, cap_entries, &query_part);
        if (rc) err = std::string("sphx_tile_query_fetch: ") + sphx_last_error(ctx);
        return rc;
    }
    // ... step 2: the records of the answered points and the kept entries come back
    int query_fetch(uint64_t cap_entries, bool nearest, bool lists) {
        const size_t n = query_part.n_points, kept = lists ? (size_t)query_part.kept : 0;
        const size_t words = n + (nearest ? 3 * n : 0) + 3 * kept;
        if (query_host.size() < words + 1) query_host.resize(words + 1);
        if (query_host_off.size() < n + 1) query_host_off.resize(n + 1);
        uint32_t* p = query_host.data();
        query_part.point = p, p += n;
        query_part.offset = query_host_off.data();
        if (nearest) {
            query_part.nearest_slot = p, p += n;
            query_part.nearest_id = p, p += n;
            query_part.nearest_dist_sq = (float*)p, p += n;
        }
        if (kept) {
            query_part.slot = p, p += kept;
            query_part.id = p, p += kept;
            query_part.dist_sq = (float*)p;
        }
        const int rc = sphx_tile_query_fetch(ctx, cap_entries, &query_part);
        if (rc) err = std::string("sphx_tile_query_fetch: ") + sphx_last_error(ctx);
        return rc;
    }
    // sphx_multi_select: the flag and scan passes; then the total; then the pairs
    std::vector<uint32_t> select_host;
    int select_enqueue(const sphx_rect* rects, uint32_t n_rects, uint32_t flags) {
        const int rc = sphx_tile_select(ctx, rects, n_rects, flags);
        if (rc) err = std::string("sphx_tile_select: ") + sphx_last_error(ctx);
        return rc;
    }
    int select_fetch(uint32_t cap, uint32_t* out_total) {
        if (select_host.size() < 2 * (size_t)cap + 2) select_host.resize(2 * (size_t)cap + 2);
        const int rc = sphx_tile_select_fetch(ctx, cap, cap ? select_host.data() : nullptr, cap ? select_host.data() + cap : nullptr, out_total);
        if (rc) err = std::string("sphx_tile_select_fetch: ") + sphx_last_error(ctx);
        return rc;
    }
};

// which layout for `world` tiles over these particles: 2x2 (2 x N/2) on 4 tiles, strips along the longer side otherwise
Layout make_layout(const sphx_multi_options& O, const sphx_params& P, int world, const float* pos, uint32_t n) {
    const float cell_inv = 1.0f / P.smoothing_length;
    std::vector<uint32_t> cx(n), cy(n);
    float lo[2] = {1e30f, 1e30f}, hi[2] = {-1e30f, -1e30f};
    for (uint32_t i = 0; i < n; ++i) {
        cx[i] = cell_coord(pos[2 * i], P.grid_min[0], cell_inv);
        cy[i] = cell_coord(pos[2 * i + 1], P.grid_min[1], cell_inv);
        for (int a = 0; a < 2; ++a) {
            lo[a] = std::min(lo[a], pos[2 * i + a]);
            hi[a] = std::max(hi[a], pos[2 * i + a]);
        }
    }
    const int axis = (hi[1] - lo[1]) > (hi[0] - lo[0]) ? 1 : 0;
    Layout L;
    const bool grid = O.layout == SPHX_LAYOUT_GRID || (O.layout == SPHX_LAYOUT_AUTO && world == 4);
    if (grid && world % 2 == 0 && world >= 4) {
        L.axis = -1;
        L.nx = axis == 1 ? 2 : world / 2;
        L.ny = world / L.nx;
        L.xcuts = quantile_cuts(cx, L.nx);
        for (int ix = 0; ix < L.nx; ++ix) {
            std::vector<uint32_t> col;
            for (uint32_t i = 0; i < n; ++i)
                if (cx[i] >= L.xcuts[ix] && cx[i] < L.xcuts[ix + 1]) col.push_back(cy[i]);
            L.ycuts.push_back(quantile_cuts(col.empty() ? cy : col, L.ny));
        }
    } else {
        L.axis = axis;
        L.xcuts = quantile_cuts(axis == 0 ? cx : cy, world);
    }
    return L;
}

}  // namespace

// ======================================================================================================================
// sphx_multi: N tiles in this process (worker threads), or one tile of a multi-process run
// ======================================================================================================================
struct sphx_multi {
    std::vector<std::unique_ptr<TileDriver>> tiles;  // in-process: all of them; rank mode: exactly one
    bool rank_mode = false;
    int world = 1;
    sphx_params P;
    sphx_multi_options O;
    std::string err;
    std::shared_ptr<LocalShared> shared;
    std::vector<float> boundary;  // host copy until the upload
    bool have_layout = false;
    Layout explicit_layout;
    bool uploaded = false;  // a sphx_multi_upload has succeeded: the contexts are tiles and hold a re-gridded particle set
    bool state_broken = false;  // a sphx_multi_state_load found a digest mismatch after the copy: the multi asks for an upload or a load
    sphx::TrackSet track;  // sphx_multi_track_set: the host tables of the set every local tile has installed (the map to the caller's order lives here only)
    std::vector<uint32_t> sample_records;  // sphx_multi_sample_points: the tiles' packed records on the host (grown on demand, kept between calls)
    MultiProbe probe;  // sphx_multi_probe_record: the recording (every tile points at it)
    uint64_t next_id = 0;  // sphx_multi_append: the id the next appended record gets (sphx_multi_edit::counter_after; the same on every rank)

    // run f(tile, index) on every tile, each on its own host thread (the tiles meet in barriers); returns the first error
    int each(const std::function<int(TileDriver&, size_t)>& f) {
        if (tiles.size() == 1) {
            const int rc = f(*tiles[0], 0);
            if (rc) err = tiles[0]->err;
            return rc;
        }
        if (shared) {  // a failure of the previous call released the tiles from their barriers: arm them again
            std::lock_guard<std::mutex> lk(shared->mu);
            shared->aborted = false;
            shared->arrived = 0;
        }
        std::vector<int> rcs(tiles.size(), 0);
        std::vector<std::thread> th;
        for (size_t r = 0; r < tiles.size(); ++r)
            th.emplace_back([&, r] {
                rcs[r] = f(*tiles[r], r);
                if (rcs[r] && shared) shared->abort();
            });
        for (auto& t : th) t.join();
        for (size_t r = 0; r < tiles.size(); ++r)
            if (rcs[r] && rcs[r] != SPHX_ERR_NOT_READY) {
                err = "tile " + std::to_string(r) + ": " + tiles[r]->err;
                return rcs[r];
            }
        for (size_t r = 0; r < tiles.size(); ++r)
            if (rcs[r]) {
                err = "tile " + std::to_string(r) + ": " + tiles[r]->err;
                return rcs[r];
            }
        return SPHX_OK;
    }
};

static std::string g_multi_error;

extern "C" {

int sphx_multi_default_options(sphx_multi_options* o) {
    if (!o) return SPHX_ERR_INVALID_ARGUMENT;
    std::memset(o, 0, sizeof(*o));
    o->halo_cells = 16;
    o->rebalance_every = 16;
    o->layout = SPHX_LAYOUT_AUTO;
    return SPHX_OK;
}

const char* sphx_multi_last_error(const sphx_multi* m) { return m ? m->err.c_str() : g_multi_error.c_str(); }

int sphx_multi_create(const sphx_params* params, const int* devices, int n_devices, const sphx_multi_options* opt, sphx_multi** out) {
    if (!params || !devices || n_devices < 1 || n_devices > 64 || !out) return SPHX_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    std::unique_ptr<sphx_multi> m(new sphx_multi());
    m->P = *params;
    if (opt)
        m->O = *opt;
    else
        sphx_multi_default_options(&m->O);
    m->world = n_devices;
    m->shared = std::make_shared<LocalShared>(n_devices);
    for (int r = 0; r < n_devices; ++r) {
        std::unique_ptr<TileDriver> t(new TileDriver());
        const int rc = t->init(*params, devices[r], m->O, std::unique_ptr<Comm>(new LocalComm(m->shared, r, devices[r])));
        if (rc) {
            g_multi_error = "tile " + std::to_string(r) + ": " + t->err;
            return rc;
        }
        t->probe = &m->probe;
        m->tiles.push_back(std::move(t));
    }
    *out = m.release();
    return SPHX_OK;
}

int sphx_multi_create_rank(const sphx_params* params, int device, const sphx_comm_ops* comm, const char* job, int rank, int world,
                           const sphx_multi_options* opt, sphx_multi** out) {
    if (!params || !out || world < 1 || rank < 0 || rank >= world) return SPHX_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    std::unique_ptr<sphx_multi> m(new sphx_multi());
    m->P = *params;
    if (opt)
        m->O = *opt;
    else
        sphx_multi_default_options(&m->O);
    m->world = world;
    m->rank_mode = true;
    std::unique_ptr<Comm> c;
    if (comm) {
        if (!comm->exchange || !comm->allreduce || comm->rank != rank || comm->world != world) return SPHX_ERR_INVALID_ARGUMENT;
        c.reset(new CallbackComm(*comm));
    } else {
        if (!job) return SPHX_ERR_INVALID_ARGUMENT;
        std::unique_ptr<RcclComm> rc(new RcclComm());
        const int e = rc->open(job, rank, world, device);
        if (e) {
            g_multi_error = rc->err;
            return e;
        }
        c = std::move(rc);
    }
    std::unique_ptr<TileDriver> t(new TileDriver());
    const int rc = t->init(*params, device, m->O, std::move(c));
    if (rc) {
        g_multi_error = t->err;
        return rc;
    }
    t->probe = &m->probe;
    m->tiles.push_back(std::move(t));
    *out = m.release();
    return SPHX_OK;
}

void sphx_multi_destroy(sphx_multi* m) { delete m; }

int sphx_multi_set_layout(sphx_multi* m, int axis, const uint32_t* cuts, uint32_t n_cuts) {
    if (!m || (axis != 0 && axis != 1) || !cuts || (int)n_cuts != m->world + 1) return SPHX_ERR_INVALID_ARGUMENT;
    m->explicit_layout = Layout();
    m->explicit_layout.axis = axis;
    m->explicit_layout.xcuts.assign(cuts, cuts + n_cuts);
    m->have_layout = true;
    return SPHX_OK;
}
int sphx_multi_set_grid_layout(sphx_multi* m, uint32_t nx, uint32_t ny, const uint32_t* xcuts, const uint32_t* ycuts) {
    if (!m || !xcuts || !ycuts || (int)(nx * ny) != m->world) return SPHX_ERR_INVALID_ARGUMENT;
    Layout L;
    L.axis = -1;
    L.nx = (int)nx;
    L.ny = (int)ny;
    L.xcuts.assign(xcuts, xcuts + nx + 1);
    for (uint32_t ix = 0; ix < nx; ++ix) L.ycuts.emplace_back(ycuts + (size_t)ix * (ny + 1), ycuts + (size_t)(ix + 1) * (ny + 1));
    m->explicit_layout = L;
    m->have_layout = true;
    return SPHX_OK;
}

int sphx_multi_set_boundary(sphx_multi* m, const float* xy, uint32_t n) {
    if (!m || (n && !xy)) return SPHX_ERR_INVALID_ARGUMENT;
    m->boundary.assign(xy, xy + 2 * (size_t)n);
    return SPHX_OK;
}

int sphx_multi_upload(sphx_multi* m, const float* pos_xy, const float* vel_xy, const uint32_t* ids, uint32_t n) {
    if (!m || (n && !pos_xy)) return SPHX_ERR_INVALID_ARGUMENT;
    const Layout L = m->have_layout ? m->explicit_layout : make_layout(m->O, m->P, m->world, pos_xy, n);
    const int rc = m->each([&](TileDriver& t, size_t) {
        return t.setup(L, pos_xy, vel_xy, ids, n, m->boundary.empty() ? nullptr : m->boundary.data(), (uint32_t)(m->boundary.size() / 2));
    });
    if (!rc) {
        m->uploaded = true;
        m->state_broken = false;
        m->next_id = sphx_multi_edit::counter_after(ids, n);
    }
    return rc;
}

int sphx_multi_step_begin(sphx_multi* m, float dt_prev, float* out_vmax) {
    if (!m || !out_vmax) return SPHX_ERR_INVALID_ARGUMENT;
    if (m->state_broken) {
        m->err = "sphx_multi_step_begin: the last sphx_multi_state_load did not complete (upload or load a state first)";
        return SPHX_ERR_NOT_READY;
    }
    std::vector<float> v(m->tiles.size(), 0.0f);
    const int rc = m->each([&](TileDriver& t, size_t k) { return t.step_begin(dt_prev, &v[k]); });
    if (rc) return rc;
    *out_vmax = v[0];  // identical on every tile (all-reduced)
    return SPHX_OK;
}

int sphx_multi_step_finish(sphx_multi* m, float dt, sphx_step_stats* out) {
    if (!m) return SPHX_ERR_INVALID_ARGUMENT;
    if (!(dt > 0) || !std::isfinite(dt)) {
        for (auto& t : m->tiles) t->in_step = false;
        m->err = "dt must be positive and finite";
        return SPHX_ERR_INVALID_ARGUMENT;
    }
    std::vector<sphx_step_stats> st(m->tiles.size());
    const int rc = m->each([&](TileDriver& t, size_t k) { return t.step_finish(dt, &st[k]); });
    if (rc) return rc;
    if (out) *out = st[0];  // iteration counts, residuals and dt are identical on every tile
    return SPHX_OK;
}

// Solver::clear_cached_data (dfsph.rs:406-412) on every tile
int sphx_multi_clear_cached(sphx_multi* m) {
    if (!m) return SPHX_ERR_INVALID_ARGUMENT;
    for (auto& t : m->tiles) {
        const int rc = sphx_clear_cached(t->ctx);
        if (rc) {
            m->err = sphx_last_error(t->ctx);
            return rc;
        }
        t->num_density_iters = 0;
        t->num_divergence_iters = 0;
    }
    return SPHX_OK;
}

// Solver::simulation_step(&mut world, &mut time_manager) in one call: phase A, the caller's TimeManager (its host mirror here:
// dfsph.rs:433 simulation_step(), :478-480 update_simulation_step), phase B — no round trip through the caller in between.
int sphx_multi_simulation_step(sphx_multi* m, sphx_timer* timer, float particle_diameter, sphx_step_stats* out_stats) {
    if (!m || !timer) return SPHX_ERR_INVALID_ARGUMENT;
    const float dt_prev = sphx_duration_as_secs_f32(sphx_timer_simulation_step_ns(timer));
    float vmax = 0;
    int rc = sphx_multi_step_begin(m, dt_prev, &vmax);
    if (rc) return rc;
    const uint64_t dt_ns = sphx_timer_update_simulation_step(timer, particle_diameter, vmax);
    return sphx_multi_step_finish(m, sphx_duration_as_secs_f32(dt_ns), out_stats);
}

int sphx_multi_simulation_steps(sphx_multi* m, sphx_timer* timer, float particle_diameter, uint32_t k, sphx_step_stats* out, uint32_t* out_done) {
    if (out_done) *out_done = 0;
    if (!m || !timer) return SPHX_ERR_INVALID_ARGUMENT;
    for (uint32_t i = 0; i < k; ++i) {
        const int rc = sphx_multi_simulation_step(m, timer, particle_diameter, out ? out + i : nullptr);
        if (rc) return rc;
        if (out_done) *out_done = i + 1;
    }
    return SPHX_OK;
}

int sphx_multi_synchronize(sphx_multi* m) {
    if (!m) return SPHX_ERR_INVALID_ARGUMENT;
    for (auto& t : m->tiles) {
        const int rc = sphx_synchronize(t->ctx);
        if (rc) return rc;
    }
    return SPHX_OK;
}

// number of particles the local tiles own (rank mode: this rank's; in-process: all)
uint64_t sphx_multi_num_owned(const sphx_multi* m) {
    uint64_t n = 0;
    if (m)
        for (auto& t : m->tiles) n += t->n_owned_local;
    return n;
}

// Owned particles of the local tiles, concatenated tile after tile; any pointer may be NULL.  *inout_n: capacity in, count out.
int sphx_multi_download(sphx_multi* m, float* pos_xy, float* vel_xy, float* density, uint32_t* ids, uint64_t* inout_n) {
    if (!m || !inout_n) return SPHX_ERR_INVALID_ARGUMENT;
    uint64_t done = 0;
    for (auto& t : m->tiles) {
        const uint32_t nl = sphx_num_particles(t->ctx);
        std::vector<float> p(2 * (size_t)nl), v(2 * (size_t)nl), d(nl);
        std::vector<uint32_t> id(nl);
        const int rc = sphx_download(t->ctx, p.data(), v.data(), d.data(), id.data());
        if (rc) {
            m->err = sphx_last_error(t->ctx);
            return rc;
        }
        for (uint32_t i = 0; i < nl; ++i) {
            if (!(id[i] >> 31)) continue;  // a ghost
            if (done < *inout_n) {
                if (pos_xy) {
                    pos_xy[2 * done] = p[2 * (size_t)i];
                    pos_xy[2 * done + 1] = p[2 * (size_t)i + 1];
                }
                if (vel_xy) {
                    vel_xy[2 * done] = v[2 * (size_t)i];
                    vel_xy[2 * done + 1] = v[2 * (size_t)i + 1];
                }
                if (density) density[done] = d[i];
                if (ids) ids[done] = id[i] & 0x7FFFFFFFu;
            }
            done += 1;
        }
    }
    const bool fits = done <= *inout_n;
    *inout_n = done;
    if (!fits) {
        m->err = "sphx_multi_download: capacity too small";
        return SPHX_ERR_CAPACITY;
    }
    return SPHX_OK;
}

int sphx_multi_info(const sphx_multi* m, sphx_multi_info_t* out) {
    if (!m || !out) return SPHX_ERR_INVALID_ARGUMENT;
    std::memset(out, 0, sizeof(*out));
    const TileDriver& t = *m->tiles[0];
    out->world = (uint32_t)m->world;
    out->local_tiles = (uint32_t)m->tiles.size();
    out->halo_now = t.halo_now;
    out->halo_max = t.halo_max;
    out->peers = (uint32_t)t.peers.size();
    out->exchanges = t.exchanges;
    out->halo_bytes_packed = t.halo_bytes_packed;
    out->halo_bytes_sent = t.halo_bytes_sent;
    out->ownership_seconds = t.ownership_seconds;
    out->rebalances = t.rebalances;
    sphx_tile_band_packs(t.ctx, &out->band_packs);
    out->n_local = t.n_local;
    out->cap_records = t.cap;
    out->grid_layout = t.layout.axis < 0;
    out->axis = t.layout.axis;
    for (auto& tp : m->tiles) {
        uint32_t np = 0;
        uint64_t ne = 0, nr = 0;
        sphx_build_stats(tp->ctx, &np, &ne, &nr);
        out->build_particles += np;
        out->neighbor_entries += ne;
        out->remote_entries += nr;
        out->owned_local += tp->n_owned_local;
    }
    std::snprintf(out->transport, sizeof(out->transport), "%s", t.comm->name());
    return SPHX_OK;
}

sphx_ctx* sphx_multi_tile_ctx(sphx_multi* m, uint32_t local_tile) { return (m && local_tile < m->tiles.size()) ? m->tiles[local_tile]->ctx : nullptr; }

// ---- fluid statistics of the tiled run (include/sphx.h, "fluid statistics of a tiled run") ---------------------------------------------
}  // extern "C"

namespace {

// local[t * cnt + k], t over the LOCAL tiles -> all[rank * cnt + k] over all `world` tiles.  In-process the local tiles are all tiles.
// Rank mode (collective, every rank with the same cnt): four 64-bit words per meeting of the ranks, each as two integers below 2^32
// (sphx_stats_merge.hpp) — every rank ends with the same bytes.
int stats_gather(sphx_multi* m, const std::vector<sphx_stats_rec>& local, size_t cnt, std::vector<sphx_stats_rec>& all) {
    all.assign((size_t)m->world * cnt, sphx_stats_rec{});
    if (!m->rank_mode) {
        std::copy(local.begin(), local.end(), all.begin());
        return SPHX_OK;
    }
    TileDriver& t = *m->tiles[0];
    Comm& comm = *t.comm;
    std::vector<double> gathered((size_t)m->world * 8);
    std::vector<double> halves((size_t)m->world * sphx_stats_host::HALVES);
    for (size_t k = 0; k < cnt; ++k) {
        double mine[sphx_stats_host::HALVES];
        sphx_stats_host::encode(local[k], mine);
        for (int part = 0; part < sphx_stats_host::HALVES / 8; ++part) {
            const int rc = comm.allgather8(mine + part * 8, gathered.data());
            if (rc) {
                m->err = "the statistics records could not be exchanged between the ranks";
                return t.fail(rc, m->err);
            }
            for (int r = 0; r < m->world; ++r)
                for (int j = 0; j < 8; ++j) halves[(size_t)r * sphx_stats_host::HALVES + part * 8 + j] = gathered[(size_t)r * 8 + j];
        }
        for (int r = 0; r < m->world; ++r) all[(size_t)r * cnt + k] = sphx_stats_host::decode(halves.data() + (size_t)r * sphx_stats_host::HALVES);
    }
    return SPHX_OK;
}

// the argument rules of sphx_fluid_stats that do not need a context (the tiles check them again; checked here so that a refused call
// has touched no tile)
const char* multi_stats_check_rects(const sphx_rect* rects, uint32_t n_rects) {
    if (n_rects > SPHX_STATS_MAX_RECTS) return "n_rects exceeds SPHX_STATS_MAX_RECTS";
    if (n_rects && !rects) return "rects is NULL with n_rects > 0";
    for (uint32_t k = 0; k < n_rects; ++k)
        if (std::isnan(rects[k].x0) || std::isnan(rects[k].y0) || std::isnan(rects[k].x1) || std::isnan(rects[k].y1)) return "rects holds a NaN bound";
    return nullptr;
}
int multi_stats_ready(sphx_multi* m, const char* fn) {
    if (!m->uploaded) {  // (the contexts become tiles with the first upload)
        m->err = std::string(fn) + ": before the first sphx_multi_upload";
        return SPHX_ERR_NOT_READY;
    }
    for (auto& t : m->tiles)
        if (t->in_step) {
            m->err = std::string(fn) + ": between sphx_multi_step_begin and sphx_multi_step_finish (finish the step first)";
            return SPHX_ERR_NOT_READY;
        }
    return SPHX_OK;
}

}  // namespace

extern "C" {

int sphx_multi_fluid_stats(sphx_multi* m, const sphx_rect* rects, uint32_t n_rects, uint32_t flags, sphx_stats_rec* out, sphx_stats_rec* out_tiles) {
    if (!m) return SPHX_ERR_INVALID_ARGUMENT;
    auto bad = [&](const std::string& what) {
        m->err = "sphx_multi_fluid_stats: " + what;
        return SPHX_ERR_INVALID_ARGUMENT;
    };
    if (!out) return bad("out is NULL");
    if (const char* b = multi_stats_check_rects(rects, n_rects)) return bad(b);
    if (flags) return bad("unknown flags bits");
    if (m->world > 64) return bad("more than 64 tiles");
    int rc;
    if ((rc = multi_stats_ready(m, "sphx_multi_fluid_stats"))) return rc;
    const size_t nrec = 1u + n_rects;
    // every local tile enqueues on its own stream and device first, then the records are collected: the tiles' passes overlap
    for (size_t k = 0; k < m->tiles.size(); ++k)
        if ((rc = m->tiles[k]->stats_enqueue(rects, n_rects))) {
            m->err = "tile " + std::to_string(k) + ": " + m->tiles[k]->err;
            return rc;
        }
    std::vector<sphx_stats_rec> local(m->tiles.size() * nrec), all;
    for (size_t k = 0; k < m->tiles.size(); ++k)
        if ((rc = m->tiles[k]->stats_fetch(n_rects, local.data() + k * nrec))) {
            m->err = "tile " + std::to_string(k) + ": " + m->tiles[k]->err;
            return rc;
        }
    if ((rc = stats_gather(m, local, nrec, all))) return rc;
    for (uint32_t r = 0; r < nrec; ++r) out[r] = sphx_stats_host::fold(all.data(), (uint32_t)m->world, nrec, r);
    if (out_tiles) std::memcpy(out_tiles, all.data(), all.size() * sizeof(sphx_stats_rec));
    return SPHX_OK;
}

int sphx_multi_stats_record(sphx_multi* m, const sphx_rect* rects, uint32_t n_rects, uint32_t max_frames, uint32_t every) {
    if (!m) return SPHX_ERR_INVALID_ARGUMENT;
    int rc;
    if ((rc = multi_stats_ready(m, "sphx_multi_stats_record"))) return rc;
    if (max_frames) {  // (checked before any tile is touched: all tiles keep the old recording or all get the new one)
        if (const char* b = multi_stats_check_rects(rects, n_rects)) {
            m->err = std::string("sphx_multi_stats_record: ") + b;
            return SPHX_ERR_INVALID_ARGUMENT;
        }
        if (every == 0) {
            m->err = "sphx_multi_stats_record: every must be >= 1";
            return SPHX_ERR_INVALID_ARGUMENT;
        }
        if ((uint64_t)max_frames * (1u + n_rects) * sizeof(sphx_stats_rec) > (64ull << 20)) {
            m->err = "sphx_multi_stats_record: max_frames * (1 + n_rects) records exceed 64 MiB per tile";
            return SPHX_ERR_CAPACITY;
        }
    }
    for (size_t k = 0; k < m->tiles.size(); ++k)
        if ((rc = sphx_tile_stats_record(m->tiles[k]->ctx, rects, n_rects, max_frames, every))) {
            m->err = "tile " + std::to_string(k) + ": " + sphx_last_error(m->tiles[k]->ctx);
            for (auto& t : m->tiles) sphx_tile_stats_record(t->ctx, nullptr, 0, 0, 1);  // no half-made recording
            return rc;
        }
    return SPHX_OK;
}

// (every tile counts the same steps and stores the same number of frames: the first local tile speaks for all)
int sphx_multi_stats_get_status(const sphx_multi* m, sphx_stats_status* out) {
    if (!m || !out) return SPHX_ERR_INVALID_ARGUMENT;
    return sphx_stats_get_status(m->tiles[0]->ctx, out);
}

int sphx_multi_stats_read(sphx_multi* m, uint32_t first_frame, uint32_t n_frames, sphx_stats_rec* out, sphx_stats_frame* info) {
    if (!m) return SPHX_ERR_INVALID_ARGUMENT;
    int rc;
    if ((rc = multi_stats_ready(m, "sphx_multi_stats_read"))) return rc;
    sphx_stats_status st;
    sphx_stats_get_status(m->tiles[0]->ctx, &st);
    if ((uint64_t)first_frame + n_frames > st.frames) {
        m->err = "sphx_multi_stats_read: first_frame + n_frames is beyond the frames recorded (sphx_multi_stats_get_status)";
        return SPHX_ERR_INVALID_ARGUMENT;
    }
    if (n_frames == 0) return SPHX_OK;
    if (!out) {
        m->err = "sphx_multi_stats_read: out is NULL";
        return SPHX_ERR_INVALID_ARGUMENT;
    }
    if (m->world > 64) {
        m->err = "sphx_multi_stats_read: more than 64 tiles";
        return SPHX_ERR_INVALID_ARGUMENT;
    }
    const size_t nrec = 1u + st.n_rects, cnt = (size_t)n_frames * nrec;
    std::vector<sphx_stats_rec> local(m->tiles.size() * cnt), all;
    for (size_t k = 0; k < m->tiles.size(); ++k)
        if ((rc = sphx_tile_stats_read(m->tiles[k]->ctx, first_frame, n_frames, local.data() + k * cnt, k == 0 ? info : nullptr))) {
            m->err = "tile " + std::to_string(k) + ": " + sphx_last_error(m->tiles[k]->ctx);
            return rc;
        }
    if ((rc = stats_gather(m, local, cnt, all))) return rc;
    for (size_t r = 0; r < cnt; ++r) out[r] = sphx_stats_host::fold(all.data(), (uint32_t)m->world, cnt, (uint32_t)r);
    return SPHX_OK;
}

}  // extern "C"

// ---- checkpoint of the tiled run (include/sphx.h, "checkpoint of a tiled run"; the device pass is csrc/sphx_multi_state.inc) ------------------
namespace {

namespace ms = sphx_multi_state;

int multi_state_ready(sphx_multi* m, const char* fn, bool need_state) {
    for (auto& t : m->tiles) {
        if (t->poisoned) {
            m->err = std::string(fn) + ": a collective step of this multi has failed (create a new one)";
            return SPHX_ERR_NOT_READY;
        }
        if (t->in_step) {
            m->err = std::string(fn) + ": between sphx_multi_step_begin and sphx_multi_step_finish (finish the step first)";
            return SPHX_ERR_NOT_READY;
        }
    }
    if (need_state && !m->uploaded) {
        m->err = std::string(fn) + (m->state_broken ? ": the last sphx_multi_state_load did not complete (upload or load a state first)" : ": before the first sphx_multi_upload or sphx_multi_state_load");
        return SPHX_ERR_NOT_READY;
    }
    return SPHX_OK;
}

// the header of the live state for the local tiles' part (digests not yet filled): n_part particles in this part
void multi_state_header(const sphx_multi* m, uint64_t n_part, ms::Header& h) {
    const TileDriver& t = *m->tiles[0];
    std::memset(&h, 0, sizeof(h));
    h.params = m->P;
    h.params.device = 0;
    ms::Scalars& s = h.s;
    s.n_part = (uint32_t)n_part;
    s.n_total = m->rank_mode ? t.n_owned_global : n_part;
    s.b = (uint32_t)(t.boundary.size() / 2);
    s.part = m->rank_mode ? (uint32_t)t.comm->rank : 0u;
    s.n_parts = m->rank_mode ? (uint32_t)m->world : 1u;
    s.num_density_iters = t.num_density_iters;
    s.num_divergence_iters = t.num_divergence_iters;
    s.last_div_iters = t.last_div_iters;
    s.last_div_warm = t.last_div_warm;
    s.steps = t.steps;
    s.tiling_invariant = sphx_get_tiling_invariant(t.ctx) ? 1u : 0u;
    s.world = (uint32_t)m->world;
    const Layout& L = t.layout;
    s.axis = L.axis >= 0 ? L.axis : -1;
    s.nx = L.axis >= 0 ? 1u : (uint32_t)L.nx;
    s.ny = L.axis >= 0 ? 1u : (uint32_t)L.ny;
    uint32_t k = 0;
    for (uint32_t c : L.xcuts) s.cuts[k++] = c;
    if (L.axis < 0)
        for (const auto& col : L.ycuts)
            for (uint32_t c : col) s.cuts[k++] = c;
    s.n_cuts = k;
    ms::layout(h);
}

// every local tile's pass: enqueued on all of them first, then the digests and counts fetched (the passes overlap)
int multi_state_pack(sphx_multi* m) {
    int rc;
    for (size_t k = 0; k < m->tiles.size(); ++k)
        if ((rc = m->tiles[k]->state_enqueue())) {
            m->err = "tile " + std::to_string(k) + ": " + m->tiles[k]->err;
            return rc;
        }
    for (size_t k = 0; k < m->tiles.size(); ++k)
        if ((rc = m->tiles[k]->state_fetch())) {
            m->err = "tile " + std::to_string(k) + ": " + m->tiles[k]->err;
            return rc;
        }
    return SPHX_OK;
}

// the local tiles' seven digests, summed mod 2^64; rank mode with `across`: summed over the ranks too — each 64-bit word as two integers
// below 2^32 (a sum of <= 64 of them is exact in a double), so that every rank ends with the same bytes
int multi_state_sum(sphx_multi* m, bool across, uint64_t* out7) {
    for (int s = 0; s < 7; ++s) {
        out7[s] = 0;
        for (auto& t : m->tiles) out7[s] += t->state_dig[s];
    }
    if (!m->rank_mode || !across || m->world == 1) return SPHX_OK;
    TileDriver& t = *m->tiles[0];
    double limbs[16] = {0}, sums[16] = {0};
    for (int s = 0; s < 7; ++s) {
        limbs[2 * s] = (double)(uint32_t)out7[s];
        limbs[2 * s + 1] = (double)(uint32_t)(out7[s] >> 32);
    }
    for (int part = 0; part < 2; ++part) {
        const int rc = t.comm->allreduce(limbs + 8 * part, 8, 0, sums + 8 * part);
        if (rc) {
            m->err = "the checkpoint digests could not be exchanged between the ranks";
            return t.fail(rc, m->err);
        }
    }
    for (int s = 0; s < 7; ++s) out7[s] = (uint64_t)sums[2 * s] + ((uint64_t)sums[2 * s + 1] << 32);
    return SPHX_OK;
}

bool read_whole_file(const std::string& path, std::vector<unsigned char>& out) {
    FILE* f = std::fopen(path.c_str(), "rb");
    if (!f) return false;
    out.clear();
    unsigned char chunk[1 << 16];
    size_t got;
    while ((got = std::fread(chunk, 1, sizeof(chunk), f)) > 0) out.insert(out.end(), chunk, chunk + got);
    const bool bad = std::ferror(f) != 0;
    std::fclose(f);
    return !bad;
}
bool file_exists(const std::string& path) {
    FILE* f = std::fopen(path.c_str(), "rb");
    if (f) std::fclose(f);
    return f != nullptr;
}
std::string part_suffix(uint32_t r, uint32_t w) {
    char b[32];
    std::snprintf(b, sizeof(b), ".r%03uof%03u", r, w);
    return b;
}

}  // namespace

extern "C" {

int sphx_multi_state_size(sphx_multi* m, uint64_t* out_bytes) {
    if (!m) return SPHX_ERR_INVALID_ARGUMENT;
    if (!out_bytes) {
        m->err = "sphx_multi_state_size: out_bytes is NULL";
        return SPHX_ERR_INVALID_ARGUMENT;
    }
    *out_bytes = 0;
    if (int rc = multi_state_ready(m, "sphx_multi_state_size", true)) return rc;
    if (m->world > (int)ms::MAX_TILES) {
        m->err = "sphx_multi_state_size: more than 64 tiles";
        return SPHX_ERR_INVALID_ARGUMENT;
    }
    if (int rc = multi_state_pack(m)) return rc;  // (the owned counts are the device's: 4 bytes per local particle would do, the pass is cheap)
    uint64_t n = 0;
    for (auto& t : m->tiles) n += t->state_owned;
    ms::Header h;
    multi_state_header(m, n, h);
    *out_bytes = h.total_bytes;
    return SPHX_OK;
}

int sphx_multi_state_save(sphx_multi* m, void* buf, uint64_t capacity, uint32_t flags, uint64_t* out_bytes) {
    if (!m) return SPHX_ERR_INVALID_ARGUMENT;
    if (out_bytes) *out_bytes = 0;
    auto bad = [&](const std::string& what) {
        m->err = "sphx_multi_state_save: " + what;
        return SPHX_ERR_INVALID_ARGUMENT;
    };
    if (flags) return bad("unknown flags bits");
    if (m->world > (int)ms::MAX_TILES) return bad("more than 64 tiles");
    int rc;
    if ((rc = multi_state_ready(m, "sphx_multi_state_save", true))) return rc;
    if ((rc = multi_state_pack(m))) return rc;
    uint64_t n = 0;
    for (auto& t : m->tiles) n += t->state_owned;
    if (n >= ms::MAX_PART) return bad("more than 2^28 particles in one part");
    ms::Header h;
    multi_state_header(m, n, h);
    if (out_bytes) *out_bytes = h.total_bytes;
    if (!buf) return bad("buf is NULL");
    if (capacity < h.total_bytes) {
        m->err = "sphx_multi_state_save: the buffer is smaller than sphx_multi_state_size";
        return SPHX_ERR_CAPACITY;
    }
    unsigned char* const b = (unsigned char*)buf;
    // the tiles' sections, tile after tile in ascending rank, every tile copying on its own stream
    uint64_t before = 0;
    for (size_t k = 0; k < m->tiles.size(); ++k) {
        TileDriver& t = *m->tiles[k];
        const sphx_tile_state_out& o = t.state_out;
        const void* src[ms::NPARTICLE_SEC] = {o.pos, o.vel, o.id, o.density, o.alpha, o.kappa, o.stiffness};
        for (uint32_t s = 0; s < ms::NPARTICLE_SEC; ++s) {
            const uint32_t w = ms::section_words(s);
            if ((rc = t.state_copy(src[s], w, b + h.sec[s].offset + before * w * 4u))) {
                m->err = "tile " + std::to_string(k) + ": " + t.err;
                return rc;
            }
        }
        before += t.state_owned;
    }
    const std::vector<float>& bnd = m->tiles[0]->boundary;
    if (!bnd.empty()) std::memcpy(b + h.sec[ms::SEC_BOUNDARY].offset, bnd.data(), bnd.size() * 4);
    for (uint32_t s = 0; s < ms::NSEC; ++s) {
        const uint64_t end = h.sec[s].offset + h.sec[s].bytes, next = s + 1 < ms::NSEC ? h.sec[s + 1].offset : h.total_bytes;
        if (next > end) std::memset(b + end, 0, next - end);
    }
    uint64_t dig[7];
    if ((rc = multi_state_sum(m, false, dig))) return rc;  // (this part's own: nothing crosses the ranks for a save)
    for (uint32_t s = 0; s < ms::NPARTICLE_SEC; ++s) h.sec[s].digest = dig[s];
    h.sec[ms::SEC_BOUNDARY].digest = sphx_state::digest_words(bnd.data(), bnd.size());
    ms::seal(h);
    std::memcpy(b, &h, sizeof(h));
    for (size_t k = 0; k < m->tiles.size(); ++k)
        if ((rc = m->tiles[k]->state_wait())) {
            m->err = "tile " + std::to_string(k) + ": " + m->tiles[k]->err;
            return rc;
        }
    return SPHX_OK;
}

int sphx_multi_state_digest(sphx_multi* m, uint64_t* out) {
    if (!m) return SPHX_ERR_INVALID_ARGUMENT;
    if (!out) {
        m->err = "sphx_multi_state_digest: out is NULL";
        return SPHX_ERR_INVALID_ARGUMENT;
    }
    int rc;
    if ((rc = multi_state_ready(m, "sphx_multi_state_digest", true))) return rc;
    if ((rc = multi_state_pack(m))) return rc;
    if ((rc = multi_state_sum(m, true, out))) return rc;
    const std::vector<float>& bnd = m->tiles[0]->boundary;
    out[ms::SEC_BOUNDARY] = sphx_state::digest_words(bnd.data(), bnd.size());
    return SPHX_OK;
}

int sphx_multi_state_load(sphx_multi* m, const void* const* parts, const uint64_t* bytes, uint32_t n_parts, uint32_t flags) {
    if (!m) return SPHX_ERR_INVALID_ARGUMENT;
    auto bad = [&](const std::string& what) {
        m->err = "sphx_multi_state_load: " + what;
        return SPHX_ERR_INVALID_ARGUMENT;
    };
    if (flags) return bad("unknown flags bits");
    if (!parts || !bytes || n_parts == 0) return bad("parts or bytes is NULL, or n_parts is 0");
    if (n_parts > ms::MAX_TILES) return bad("more than 64 parts");
    if (m->world > (int)ms::MAX_TILES) return bad("more than 64 tiles");
    int rc;
    if ((rc = multi_state_ready(m, "sphx_multi_state_load", false))) return rc;
    // ---- host-side validation: nothing of the multi changes before it has passed --------------------------------------------------------
    std::vector<ms::Header> hs(n_parts);
    std::string why;
    for (uint32_t i = 0; i < n_parts; ++i)
        if (!ms::validate(parts[i], bytes[i], &hs[i], &why)) return bad("part " + std::to_string(i) + ": " + why);
    if (!ms::validate_set(hs.data(), n_parts, &why)) return bad(why);
    const ms::Header& h0 = hs[0];
    if (const char* field = sphx_state::params_mismatch(h0.params, m->P))
        return bad(std::string("the checkpoint was saved under other params than this multi's; first field that differs: ") + field);
    for (auto& t : m->tiles)
        if ((h0.s.tiling_invariant != 0) != (sphx_get_tiling_invariant(t->ctx) != 0))
            return bad(h0.s.tiling_invariant ? "the checkpoint was saved in tiling-invariant mode, this multi's tiles are not in it"
                                             : "this multi's tiles are in tiling-invariant mode, the checkpoint was not saved in it");
    // the parts in the order of their index; ids, padding and the boundary of each
    std::vector<uint32_t> order(n_parts);
    for (uint32_t i = 0; i < n_parts; ++i) order[hs[i].s.part] = i;  // (validate_set: a permutation of 0 .. n_parts - 1)
    const uint64_t n = h0.s.n_total;
    const uint32_t nb = h0.s.b;
    for (uint32_t i = 0; i < n_parts; ++i) {
        const unsigned char* p = (const unsigned char*)parts[i];
        const ms::Header& h = hs[i];
        if (!ms::padding_is_zero(p, h)) return bad("part " + std::to_string(i) + ": padding bytes are not zero");
        const ms::Section& sb = h.sec[ms::SEC_BOUNDARY];
        std::vector<float> bnd((size_t)nb * 2);
        if (sb.bytes) std::memcpy(bnd.data(), p + sb.offset, sb.bytes);
        if (sphx_state::digest_words(bnd.data(), sb.bytes / 4u) != sb.digest) return bad("part " + std::to_string(i) + ": digest mismatch in section boundary");
        const ms::Section& si = h.sec[SPHX_MULTI_STATE_SEC_PARTICLE_ID];
        for (uint64_t k = 0; k < h.s.n_part; ++k) {
            uint32_t id;
            std::memcpy(&id, p + si.offset + 4 * k, 4);
            if (id >> 31) return bad("part " + std::to_string(i) + ": a particle id is not below 2^31");
        }
    }
    // the global arrays, parts in ascending index (as sphx_multi_upload is given them)
    std::vector<float> pos(2 * n), vel(2 * n), kap(n), stf(n), bnd((size_t)nb * 2);
    std::vector<uint32_t> ids(n);
    uint64_t want[7] = {0};
    {
        uint64_t at = 0;
        for (uint32_t r = 0; r < n_parts; ++r) {
            const unsigned char* p = (const unsigned char*)parts[order[r]];
            const ms::Header& h = hs[order[r]];
            const uint64_t k = h.s.n_part;
            if (k) {
                std::memcpy(pos.data() + 2 * at, p + h.sec[SPHX_MULTI_STATE_SEC_POSITIONS].offset, 8 * k);
                std::memcpy(vel.data() + 2 * at, p + h.sec[SPHX_MULTI_STATE_SEC_VELOCITIES].offset, 8 * k);
                std::memcpy(ids.data() + at, p + h.sec[SPHX_MULTI_STATE_SEC_PARTICLE_ID].offset, 4 * k);
                std::memcpy(kap.data() + at, p + h.sec[SPHX_MULTI_STATE_SEC_KAPPA].offset, 4 * k);
                std::memcpy(stf.data() + at, p + h.sec[SPHX_MULTI_STATE_SEC_STIFFNESS].offset, 4 * k);
            }
            at += k;
            for (int s = 0; s < 7; ++s) want[s] += h.sec[s].digest;
        }
        const ms::Section& sb = h0.sec[ms::SEC_BOUNDARY];
        if (sb.bytes) std::memcpy(bnd.data(), (const unsigned char*)parts[0] + sb.offset, sb.bytes);
    }
    // the layout: an explicit one; else the saver's, if it had as many tiles; else the quantile layout over the checkpoint's positions
    Layout L;
    if (m->have_layout) {
        L = m->explicit_layout;
    } else if ((int)h0.s.world == m->world) {
        const ms::Scalars& s = h0.s;
        L.axis = s.axis;
        if (s.axis >= 0) {
            L.xcuts.assign(s.cuts, s.cuts + s.n_cuts);
        } else {
            L.nx = (int)s.nx;
            L.ny = (int)s.ny;
            L.xcuts.assign(s.cuts, s.cuts + s.nx + 1);
            for (uint32_t ix = 0; ix < s.nx; ++ix) L.ycuts.emplace_back(s.cuts + s.nx + 1 + ix * (s.ny + 1), s.cuts + s.nx + 1 + (ix + 1) * (s.ny + 1));
        }
    } else {
        L = make_layout(m->O, m->P, m->world, pos.data(), (uint32_t)n);
    }
    if (L.world() != m->world) return bad("the layout set for this multi and its tile count disagree");
    // ---- from here on the multi changes -----------------------------------------------------------------------------------------------------
    auto broken = [&](int code) {  // the tiles hold half a state: the multi asks for an upload or a load
        m->uploaded = false;
        m->state_broken = true;
        return code;
    };
    m->boundary = bnd;
    rc = m->each([&](TileDriver& t, size_t) {
        const int e = t.setup(L, pos.data(), vel.data(), ids.data(), (uint32_t)n, bnd.empty() ? nullptr : bnd.data(), nb, kap.data(), stf.data());
        // (setup ends with the one halo exchange and re-grid; it left the counts of a fresh upload)
        t.num_density_iters = h0.s.num_density_iters;
        t.num_divergence_iters = h0.s.num_divergence_iters;
        t.last_div_iters = h0.s.last_div_iters;
        t.last_div_warm = h0.s.last_div_warm;
        t.steps = h0.s.steps;
        return e;
    });
    if (rc) return broken(rc);
    m->uploaded = true;
    m->state_broken = false;
    m->next_id = sphx_multi_edit::counter_after(ids.data(), n);
    // what arrived, digested where it now lives
    uint64_t got[7];
    if ((rc = multi_state_pack(m)) || (rc = multi_state_sum(m, true, got))) return broken(rc);
    for (uint32_t s : {(uint32_t)SPHX_MULTI_STATE_SEC_POSITIONS, (uint32_t)SPHX_MULTI_STATE_SEC_VELOCITIES, (uint32_t)SPHX_MULTI_STATE_SEC_PARTICLE_ID,
                       (uint32_t)SPHX_MULTI_STATE_SEC_KAPPA, (uint32_t)SPHX_MULTI_STATE_SEC_STIFFNESS})
        if (got[s] != want[s]) return broken(bad(std::string("digest mismatch in section ") + ms::section_name(s) + " (upload or load a state again)"));
    return SPHX_OK;
}

int sphx_multi_state_save_file(sphx_multi* m, const char* path) {
    if (!m) return SPHX_ERR_INVALID_ARGUMENT;
    if (!path) {
        m->err = "sphx_multi_state_save_file: path is NULL";
        return SPHX_ERR_INVALID_ARGUMENT;
    }
    uint64_t bytes = 0;
    int rc;
    if ((rc = sphx_multi_state_size(m, &bytes))) return rc;
    std::vector<unsigned char> blob(bytes);
    if ((rc = sphx_multi_state_save(m, blob.data(), bytes, 0u, nullptr))) return rc;
    const std::string dst = std::string(path) + (m->rank_mode ? part_suffix((uint32_t)m->tiles[0]->comm->rank, (uint32_t)m->world) : std::string());
    const std::string tmp = dst + ".tmp";
    FILE* f = std::fopen(tmp.c_str(), "wb");
    bool ok = f != nullptr;
    if (ok) {
        ok = std::fwrite(blob.data(), 1, blob.size(), f) == blob.size();
        ok = std::fclose(f) == 0 && ok;
    }
    if (ok) ok = std::rename(tmp.c_str(), dst.c_str()) == 0;
    if (!ok) {
        const std::string e = std::strerror(errno);
        std::remove(tmp.c_str());
        m->err = "sphx_multi_state_save_file: cannot write " + dst + ": " + e;
        return SPHX_ERR_INVALID_ARGUMENT;
    }
    return SPHX_OK;
}

int sphx_multi_state_load_file(sphx_multi* m, const char* path) {
    if (!m) return SPHX_ERR_INVALID_ARGUMENT;
    auto bad = [&](const std::string& what) {
        m->err = "sphx_multi_state_load_file: " + what;
        return SPHX_ERR_INVALID_ARGUMENT;
    };
    if (!path) return bad("path is NULL");
    std::vector<std::vector<unsigned char>> files;
    std::vector<const void*> parts;
    std::vector<uint64_t> bytes;
    if (file_exists(path)) {
        files.emplace_back();
        if (!read_whole_file(path, files[0])) return bad(std::string("cannot read ") + path);
        std::vector<std::pair<uint64_t, uint64_t>> pieces;
        std::string why;
        if (files[0].empty() || !ms::split_parts(files[0].data(), files[0].size(), &pieces, &why)) return bad(files[0].empty() ? "the file is empty" : why);
        for (const auto& pc : pieces) {
            parts.push_back(files[0].data() + pc.first);
            bytes.push_back(pc.second);
        }
    } else {
        uint32_t w = 0;
        for (uint32_t k = 1; k <= ms::MAX_TILES && !w; ++k)
            if (file_exists(std::string(path) + part_suffix(0, k))) w = k;
        if (!w) return bad(std::string("neither ") + path + " nor " + path + ".r000ofWWW exists");
        files.resize(w);
        for (uint32_t r = 0; r < w; ++r) {
            const std::string name = std::string(path) + part_suffix(r, w);
            if (!read_whole_file(name, files[r]) || files[r].empty()) return bad("the set of part files is incomplete: cannot read " + name);
            parts.push_back(files[r].data());
            bytes.push_back(files[r].size());
        }
    }
    return sphx_multi_state_load(m, parts.data(), bytes.data(), (uint32_t)parts.size(), 0u);
}

}  // extern "C"

// ---- emitting and draining fluid in a tiled run (include/sphx.h; the device passes are csrc/sphx_multi_edit.inc) ------------------------------
extern "C" {

int sphx_multi_remove(sphx_multi* m, const sphx_rect* rects, uint32_t n_rects, uint32_t flags, uint64_t* out_removed) {
    if (!m) return SPHX_ERR_INVALID_ARGUMENT;
    if (out_removed) *out_removed = 0;
    auto bad = [&](const std::string& what) {
        m->err = "sphx_multi_remove: " + what;
        return SPHX_ERR_INVALID_ARGUMENT;
    };
    // sphx_remove's argument rules, checked here so that a refused call has touched no tile
    if (n_rects > SPHX_REMOVE_MAX_RECTS) return bad("n_rects is larger than SPHX_REMOVE_MAX_RECTS");
    if (n_rects && !rects) return bad("rects is NULL with n_rects > 0");
    if (flags & ~(uint32_t)SPHX_REMOVE_OUTSIDE) return bad("unknown flags bits");
    for (uint32_t k = 0; k < n_rects; ++k)
        if (std::isnan(rects[k].x0) || std::isnan(rects[k].y0) || std::isnan(rects[k].x1) || std::isnan(rects[k].y1)) return bad("a rectangle bound is NaN");
    int rc;
    if ((rc = multi_state_ready(m, "sphx_multi_remove", true))) return rc;
    // every local tile enqueues on its own stream and device first, then the counts are collected: the tiles' passes overlap.  A failure
    // here is this process's own (the arguments and the state rules are the same everywhere): it is kept until the ranks have met
    int local_rc = SPHX_OK;
    for (size_t k = 0; k < m->tiles.size() && !local_rc; ++k)
        if ((local_rc = m->tiles[k]->edit_remove_enqueue(rects, n_rects, flags))) m->err = "tile " + std::to_string(k) + ": " + m->tiles[k]->err;
    double local = 0.0, total = 0.0;
    for (size_t k = 0; k < m->tiles.size() && !local_rc; ++k) {
        if ((local_rc = m->tiles[k]->edit_remove_fetch())) m->err = "tile " + std::to_string(k) + ": " + m->tiles[k]->err;
        local += (double)m->tiles[k]->edit_removed;
    }
    if (m->rank_mode) {
        // the one collective of the decision, reached by every rank whatever its own count and whether or not its own pass failed (the
        // second word says so: then every rank returns an error together)
        TileDriver& t = *m->tiles[0];
        double in[2] = {local, local_rc ? 1.0 : 0.0}, out[2] = {0.0, 0.0};
        if ((rc = t.comm->allreduce(in, 2, 0, out))) {
            m->err = "sphx_multi_remove: the removed counts could not be summed over the ranks";
            return t.fail(rc, m->err);
        }
        if (out[1] > 0.0) {
            if (!local_rc) m->err = "sphx_multi_remove: another rank's marking pass failed";
            return local_rc ? local_rc : SPHX_ERR_HIP;  // (every rank has left the all-reduce: nobody is waiting for this one)
        }
        total = out[0];
    } else {
        if (local_rc) return local_rc;
        total = local;
    }
    const uint64_t removed = (uint64_t)total;
    if (out_removed) *out_removed = removed;
    if (removed == 0) return SPHX_OK;  // the multi is as it was
    return m->each([&](TileDriver& t, size_t) { return t.edit_remove_finish(removed); });
}

int sphx_multi_append(sphx_multi* m, const float* pos_xy, const float* vel_xy, uint32_t n_new, uint32_t* out_first_id) {
    if (!m) return SPHX_ERR_INVALID_ARGUMENT;
    if (n_new && !pos_xy) {
        m->err = "sphx_multi_append: pos_xy is NULL with n_new > 0";
        return SPHX_ERR_INVALID_ARGUMENT;
    }
    int rc;
    if ((rc = multi_state_ready(m, "sphx_multi_append", true))) return rc;
    const uint32_t bad_at = sphx_multi_edit::first_nonfinite(pos_xy, n_new);
    if (bad_at != n_new) {
        m->err = "sphx_multi_append: the position of record " + std::to_string(bad_at) + " is not finite (a NaN x is the mark of a retired record)";
        return SPHX_ERR_INVALID_ARGUMENT;
    }
    uint32_t first_id = 0;
    uint64_t counter = m->next_id;
    if (!sphx_multi_edit::take_ids(counter, n_new, &first_id)) {
        if (out_first_id) *out_first_id = first_id;
        m->err = "sphx_multi_append: a particle id would reach 2^31 (ids are not reused within a run; bit 31 marks the owner inside a tile)";
        return SPHX_ERR_CAPACITY;
    }
    if (out_first_id) *out_first_id = first_id;
    if (n_new == 0) return SPHX_OK;
    // the owner of every record under the CURRENT layout (the same on every tile and rank: the layout is)
    const TileDriver& t0 = *m->tiles[0];
    std::vector<sphx_multi_edit::CellRect> rects;
    for (const Rect& r : t0.layout.rects()) rects.push_back(sphx_multi_edit::CellRect{r.x0, r.x1, r.y0, r.y1});
    std::vector<int> owner;
    sphx_multi_edit::route(pos_xy, n_new, t0.grid_min, t0.cell_inv, rects.data(), (int)rects.size(), owner);
    for (uint32_t k = 0; k < n_new; ++k)
        if (owner[k] < 0) {  // (cannot happen: a layout's rectangles cover the cell range)
            m->err = "sphx_multi_append: no tile's rectangle holds record " + std::to_string(k);
            return SPHX_ERR_INVALID_ARGUMENT;
        }
    m->next_id = counter;
    return m->each([&](TileDriver& t, size_t) { return t.edit_append(pos_xy, vel_xy, n_new, first_id, owner); });
}

}  // extern "C"

// ---- picture of the tiled run (include/sphx.h, "picture of a tiled run"; the device passes are csrc/sphx_render.inc) ---------------------------
namespace {

// The merged layer of the local tiles into acc (host, full size; acc.rgba null: no colours): every tile enqueues its window on its own
// stream and device, then the windows are copied back and folded in ascending tile rank.  Outside its window a tile shows nothing.
int multi_render_layers(sphx_multi* m, const char* fn, const sphx_render_view* view, const sphx_render_layer& acc) {
    const size_t npix = (size_t)view->width * view->height;
    const bool rgba = acc.rgba != nullptr;
    for (size_t p = 0; p < npix; ++p) {
        acc.key[p] = 0u;
        acc.owner[p] = (uint32_t)SPHX_RENDER_NONE;
        if (rgba) std::memcpy(acc.rgba + 4 * p, view->background, 4);
    }
    int rc;
    for (size_t k = 0; k < m->tiles.size(); ++k)
        if ((rc = m->tiles[k]->render_enqueue(view, rgba))) {
            m->err = std::string(fn) + ": tile " + std::to_string(k) + ": " + m->tiles[k]->err;
            return rc;
        }
    for (size_t k = 0; k < m->tiles.size(); ++k)
        if ((rc = m->tiles[k]->render_fetch(rgba))) {
            m->err = std::string(fn) + ": tile " + std::to_string(k) + ": " + m->tiles[k]->err;
            return rc;
        }
    for (size_t k = 0; k < m->tiles.size(); ++k) {
        TileDriver& t = *m->tiles[k];
        if ((rc = t.render_wait())) {
            m->err = std::string(fn) + ": tile " + std::to_string(k) + ": " + t.err;
            return rc;
        }
        if (!t.render_pixels()) continue;
        const uint32_t* w = t.render_win;
        if (w[0] > w[1] || w[1] > view->width || w[2] > w[3] || w[3] > view->height) {  // (cannot happen: the window is clipped to the image)
            m->err = std::string(fn) + ": tile " + std::to_string(k) + " returned a window outside the image";
            return SPHX_ERR_HIP;
        }
        const sphx_render_layer src{t.render_key.data(), t.render_owner.data(), rgba ? (uint8_t*)t.render_rgba.data() : nullptr};
        sphx_render_host::fold_window(acc, view->width, src, w[0], w[1], w[2], w[3]);
    }
    return SPHX_OK;
}

// the rules both calls share, in sphx_render's order: SPHX_OK go on, RENDER_NOOP a successful no-op (no pixels), else the error code
constexpr int RENDER_NOOP = -1;  // (no status code is negative)
int multi_render_ready(sphx_multi* m, const char* fn, const sphx_render_view* view, bool has_out, bool no_output, const char* none_msg, uint32_t flags) {
    auto bad = [&](const std::string& what) {
        m->err = std::string(fn) + ": " + what;
        return SPHX_ERR_INVALID_ARGUMENT;
    };
    if (!view) return bad("view is NULL");
    if (!has_out) return bad("out is NULL");
    if (no_output) return bad(none_msg);
    if (flags) return bad("unknown flags bits");
    if (m->world > 64) return bad("more than 64 tiles");
    if (const char* b = sphx::render_view_error(view, m->P.smoothing_length)) return bad(b);
    if ((uint64_t)view->width * view->height == 0) return RENDER_NOOP;
    return multi_state_ready(m, fn, true);
}

}  // namespace

extern "C" {

int sphx_render_merge(uint32_t width, uint32_t height, const sphx_render_layer* layers, uint32_t n_layers, const sphx_render_layer* out) {
    if (const char* b = sphx_render_host::merge_error(width, height, layers, n_layers, out)) {
        g_multi_error = std::string("sphx_render_merge: ") + b;  // (no object to hang the message on: sphx_multi_last_error(NULL))
        return SPHX_ERR_INVALID_ARGUMENT;
    }
    sphx_render_host::merge(width, height, layers, n_layers, out);
    return SPHX_OK;
}

int sphx_multi_render_layer(sphx_multi* m, const sphx_render_view* view, uint32_t flags, const sphx_render_layer* out) {
    if (!m) return SPHX_ERR_INVALID_ARGUMENT;
    const char* const fn = "sphx_multi_render_layer";
    int rc;
    if ((rc = multi_render_ready(m, fn, view, out != nullptr, out && !out->key && !out->owner && !out->rgba, "out requests no output (key, owner and rgba are NULL)", flags)))
        return rc == RENDER_NOOP ? SPHX_OK : rc;
    // (the fold needs keys and owners whatever the caller asks for)
    const size_t npix = (size_t)view->width * view->height;
    std::vector<uint32_t> key, owner;
    if (!out->key) key.resize(npix);
    if (!out->owner) owner.resize(npix);
    const sphx_render_layer acc{out->key ? out->key : key.data(), out->owner ? out->owner : owner.data(), out->rgba};
    return multi_render_layers(m, fn, view, acc);
}

int sphx_multi_render(sphx_multi* m, const sphx_render_view* view, uint32_t flags, const sphx_render_out* out) {
    if (!m) return SPHX_ERR_INVALID_ARGUMENT;
    const char* const fn = "sphx_multi_render";
    if (m->rank_mode) {  // (whatever the other arguments say: this process holds one tile of the run)
        m->err = std::string(fn) + ": not available in rank mode (one tile per process): take each rank's sphx_multi_render_layer, move the layers with "
                                   "your own transport and merge them with sphx_render_merge";
        return SPHX_ERR_INVALID_ARGUMENT;
    }
    int rc;
    if ((rc = multi_render_ready(m, fn, view, out != nullptr, out && !out->rgba && !out->owner, "out requests no output (rgba and owner are NULL)", flags)))
        return rc == RENDER_NOOP ? SPHX_OK : rc;
    const size_t npix = (size_t)view->width * view->height;
    std::vector<uint32_t> key(npix), owner;
    if (!out->owner) owner.resize(npix);
    const sphx_render_layer acc{key.data(), out->owner ? out->owner : owner.data(), out->rgba};
    return multi_render_layers(m, fn, view, acc);
}

}  // extern "C"

// ---- following particles by id in a tiled run (include/sphx.h, "following particles by id in a tiled run"; the device passes are
// csrc/sphx_track.inc, the fold is csrc/sphx_track_merge.hpp) ---------------------------------------------------------------------------
namespace {

namespace th = sphx_track_host;

uint32_t track_tile_rank(const sphx_multi* m, size_t k) { return m->rank_mode ? (uint32_t)m->tiles[0]->comm->rank : (uint32_t)k; }

int track_bad(sphx_multi* m, const char* fn, const char* what) {
    m->err = std::string(fn) + ": " + what;
    return SPHX_ERR_INVALID_ARGUMENT;
}
int track_tile_failed(sphx_multi* m, size_t k, int rc) {
    m->err = "tile " + std::to_string(k) + ": " + sphx_last_error(m->tiles[k]->ctx);
    return rc;
}
const char* track_out_error(const sphx_multi_track_out* out, uint32_t flags) {
    if (!out) return "out is NULL";
    if (!out->tile && !out->slot && !out->pos && !out->vel && !out->density) return "out requests no output (every pointer is NULL)";
    if (flags) return "unknown flags bits";
    return nullptr;
}

// the caller's arrays from entry `at` on as the accumulator of the fold; tile and slot are lent where the caller has none
struct TrackAcc {
    std::vector<uint32_t> tile, slot;
    th::Acc acc;
    TrackAcc(const sphx_multi_track_out& o, size_t at, size_t n) {
        if (!o.tile) tile.resize(n);
        if (!o.slot) slot.resize(n);
        acc.tile = o.tile ? o.tile + at : tile.data();
        acc.slot = o.slot ? o.slot + at : slot.data();
        acc.pos = o.pos ? (uint32_t*)o.pos + 2 * at : nullptr;
        acc.vel = o.vel ? (uint32_t*)o.vel + 2 * at : nullptr;
        acc.density = o.density ? (uint32_t*)o.density + at : nullptr;
    }
};

}  // namespace

extern "C" {

int sphx_track_merge(uint32_t n, const sphx_multi_track_out* parts, uint32_t n_parts, const sphx_multi_track_out* out, uint32_t* out_present) {
    if (const char* b = th::merge_error(n, parts, n_parts, out)) {
        g_multi_error = std::string("sphx_track_merge: ") + b;  // (no object to hang the message on: sphx_multi_last_error(NULL))
        return SPHX_ERR_INVALID_ARGUMENT;
    }
    TrackAcc a(*out, 0, n);
    th::merge(n, parts, n_parts, a.acc);
    if (out_present) *out_present = th::count_present(a.acc.tile, n);
    return SPHX_OK;
}

int sphx_track_merge_frames(uint64_t n, const float* const* parts, const uint32_t* const* parts_tile, uint32_t n_parts, float* out, uint32_t* out_tile) {
    if (const char* b = th::merge_frames_error(n, parts, parts_tile, n_parts, out)) {
        g_multi_error = std::string("sphx_track_merge_frames: ") + b;
        return SPHX_ERR_INVALID_ARGUMENT;
    }
    std::vector<uint32_t> tile;
    if (!out_tile) tile.resize((size_t)n);
    th::merge_frames(n, parts, parts_tile, n_parts, out, out_tile ? out_tile : tile.data());
    return SPHX_OK;
}

int sphx_multi_track_set(sphx_multi* m, const uint32_t* ids, uint32_t n_ids) {
    if (!m) return SPHX_ERR_INVALID_ARGUMENT;
    const char* const fn = "sphx_multi_track_set";
    if (const char* b = sphx::track_check_ids(ids, n_ids)) return track_bad(m, fn, b);
    int rc;
    if ((rc = multi_state_ready(m, fn, true))) return rc;
    sphx::TrackSet s = sphx::track_build(ids, n_ids);  // built once: every tile gets the same tables
    for (size_t k = 0; k < m->tiles.size(); ++k)
        if ((rc = sphx_tile_track_install(m->tiles[k]->ctx, s.table.data(), s.filter.data(), s.unique(), s.log2_bits))) {
            track_tile_failed(m, k, rc);
            for (auto& t : m->tiles) sphx_tile_track_install(t->ctx, nullptr, nullptr, 0, 0);  // no half-made set
            m->track = sphx::TrackSet();
            return rc;
        }
    m->track = std::move(s);
    return SPHX_OK;
}

int sphx_multi_track_fetch(sphx_multi* m, uint32_t flags, const sphx_multi_track_out* out) {
    if (!m) return SPHX_ERR_INVALID_ARGUMENT;
    const char* const fn = "sphx_multi_track_fetch";
    if (const char* b = track_out_error(out, flags)) return track_bad(m, fn, b);
    int rc;
    if ((rc = multi_state_ready(m, fn, true))) return rc;
    const uint32_t n = m->track.m(), u = m->track.unique();
    if (!n) return SPHX_OK;
    // every local tile enqueues on its own stream and device first, then the parts are collected: the tiles' passes overlap
    for (size_t k = 0; k < m->tiles.size(); ++k)
        if ((rc = sphx_tile_track_fetch_enqueue(m->tiles[k]->ctx))) return track_tile_failed(m, k, rc);
    // the answer over the distinct ids, with the arrays the caller asked for
    std::vector<uint32_t> a_tile(u), a_slot(u), a_pos(out->pos ? 2 * (size_t)u : 0), a_vel(out->vel ? 2 * (size_t)u : 0), a_den(out->density ? u : 0);
    const th::Acc au{a_tile.data(), a_slot.data(), out->pos ? a_pos.data() : nullptr, out->vel ? a_vel.data() : nullptr, out->density ? a_den.data() : nullptr};
    th::fill_absent(au, u);
    std::vector<uint32_t> slot(u), xyvv(4 * (size_t)u), den(u);
    for (size_t k = 0; k < m->tiles.size(); ++k) {
        if ((rc = sphx_tile_track_fetch(m->tiles[k]->ctx, slot.data(), (float*)xyvv.data(), (float*)den.data()))) return track_tile_failed(m, k, rc);
        th::fold_unique(au, track_tile_rank(m, k), u, slot.data(), xyvv.data(), den.data());
    }
    TrackAcc a(*out, 0, n);
    th::expand(a.acc, au, m->track.map.data(), n);
    return SPHX_OK;
}

int sphx_multi_download_by_id(sphx_multi* m, uint32_t first_id, uint32_t count, uint32_t flags, const sphx_multi_track_out* out, uint32_t* out_present) {
    if (!m) return SPHX_ERR_INVALID_ARGUMENT;
    const char* const fn = "sphx_multi_download_by_id";
    if (const char* b = track_out_error(out, flags)) return track_bad(m, fn, b);
    if (const char* b = sphx::track_check_range(first_id, count)) return track_bad(m, fn, b);
    int rc;
    if ((rc = multi_state_ready(m, fn, true))) return rc;
    if (out_present) *out_present = 0;
    uint32_t present = 0;
    std::vector<uint32_t> records;
    std::vector<uint32_t> caps(m->tiles.size());
    for (uint64_t w0 = 0; w0 < count; w0 += th::WINDOW) {
        const uint32_t wc = (uint32_t)std::min<uint64_t>(count - w0, th::WINDOW);
        const uint32_t wfirst = first_id + (uint32_t)w0;
        // a tile's buffer follows what it owns, not the window: the tiles together return about one record per particle of the window
        for (size_t k = 0; k < m->tiles.size(); ++k) {
            caps[k] = (uint32_t)std::min<uint64_t>(wc, m->tiles[k]->n_owned_local);
            if ((rc = sphx_tile_track_window_enqueue(m->tiles[k]->ctx, wfirst, wc, caps[k]))) return track_tile_failed(m, k, rc);
        }
        TrackAcc a(*out, (size_t)w0, wc);
        th::fill_absent(a.acc, wc);
        for (size_t k = 0; k < m->tiles.size(); ++k) {
            records.resize(th::HEADER_WORDS + (size_t)caps[k] * th::RECORD_WORDS);
            uint32_t n_rec = 0;
            if ((rc = sphx_tile_track_window_fetch(m->tiles[k]->ctx, records.data(), &n_rec))) return track_tile_failed(m, k, rc);
            if (th::scatter_records(a.acc, track_tile_rank(m, k), wc, records.data() + th::HEADER_WORDS, n_rec)) {
                m->err = std::string(fn) + ": tile " + std::to_string(k) + " returned a record outside the window";
                return SPHX_ERR_HIP;
            }
        }
        present += th::count_present(a.acc.tile, wc);
    }
    if (out_present) *out_present = present;
    return SPHX_OK;
}

int sphx_multi_track_record(sphx_multi* m, uint32_t max_frames, uint32_t every) {
    if (!m) return SPHX_ERR_INVALID_ARGUMENT;
    const char* const fn = "sphx_multi_track_record";
    int rc;
    if ((rc = multi_state_ready(m, fn, true))) return rc;
    if (max_frames) {  // (checked before any tile is touched: all tiles keep the old recording or all get the new one)
        if (every == 0) return track_bad(m, fn, "every is 0");
        if ((uint64_t)max_frames * m->track.unique() * th::FRAME_ENTRY_BYTES > th::RECORD_MAX_BYTES) {
            m->err = std::string(fn) + ": max_frames * (distinct ids) * 20 bytes is more than 1 GiB per tile";
            return SPHX_ERR_CAPACITY;
        }
        if (!m->track.m()) {
            m->err = std::string(fn) + ": the tracked set is empty (call sphx_multi_track_set first)";
            return SPHX_ERR_NOT_READY;
        }
    }
    for (size_t k = 0; k < m->tiles.size(); ++k)
        if ((rc = sphx_tile_track_record(m->tiles[k]->ctx, max_frames, every))) {
            track_tile_failed(m, k, rc);
            for (auto& t : m->tiles) sphx_tile_track_record(t->ctx, 0, 1);  // no half-made recording
            return rc;
        }
    return SPHX_OK;
}

// (every tile counts the same steps and stores the same number of frames: the first local tile speaks for all; m is the caller's)
int sphx_multi_track_get_status(const sphx_multi* m, sphx_track_status* out) {
    if (!m || !out) return SPHX_ERR_INVALID_ARGUMENT;
    const int rc = sphx_track_get_status(m->tiles[0]->ctx, out);
    out->m = m->track.m();
    return rc;
}

int sphx_multi_track_read(sphx_multi* m, uint32_t first_frame, uint32_t n_frames, uint32_t flags, float* out, uint32_t* out_tile) {
    if (!m) return SPHX_ERR_INVALID_ARGUMENT;
    const char* const fn = "sphx_multi_track_read";
    if (flags) return track_bad(m, fn, "unknown flags bits");
    int rc;
    if ((rc = multi_state_ready(m, fn, true))) return rc;
    sphx_track_status st;
    sphx_track_get_status(m->tiles[0]->ctx, &st);
    if ((uint64_t)first_frame + n_frames > st.frames) return track_bad(m, fn, "first_frame + n_frames is beyond the frames recorded (sphx_multi_track_get_status)");
    if (n_frames == 0) return SPHX_OK;
    if (!out) return track_bad(m, fn, "out is NULL");
    const uint32_t n = m->track.m(), u = m->track.unique();
    const size_t cnt = (size_t)n_frames * u;
    std::vector<uint32_t> xyvv(4 * cnt, th::ABSENT_WORD), tile(cnt, th::ABSENT), slot(cnt, th::ABSENT), t_xyvv(4 * cnt), t_slot(cnt);
    for (size_t k = 0; k < m->tiles.size(); ++k) {
        if ((rc = sphx_tile_track_read(m->tiles[k]->ctx, first_frame, n_frames, (float*)t_xyvv.data(), t_slot.data()))) return track_tile_failed(m, k, rc);
        th::fold_frames_unique(xyvv.data(), tile.data(), slot.data(), track_tile_rank(m, k), cnt, t_xyvv.data(), t_slot.data());
    }
    const uint32_t* const map = m->track.map.data();
    for (uint32_t f = 0; f < n_frames; ++f)
        for (uint32_t k = 0; k < n; ++k) {
            const size_t src = (size_t)f * u + map[k], dst = (size_t)f * n + k;
            std::memcpy(out + 4 * dst, xyvv.data() + 4 * src, 16);
            if (out_tile) out_tile[dst] = tile[src];
        }
    return SPHX_OK;
}

}  // extern "C"

// ---- sampling the fields of a tiled run (include/sphx.h, "sampling the fields of a tiled run"; the device passes are
// csrc/sphx_sample.inc, the lattice windows and the fold csrc/sphx_sample_window.hpp) ----------------------------------------------------
namespace {

namespace sh = sphx_sample_host;

int sample_bad(sphx_multi* m, const char* fn, const char* what) {
    m->err = std::string(fn) + ": " + what;
    return SPHX_ERR_INVALID_ARGUMENT;
}
uint32_t sample_fields(const sphx_multi_sample_out* o) {
    return (o->density ? (uint32_t)SPHX_SAMPLE_FIELD_DENSITY : 0u) | (o->fraction ? (uint32_t)SPHX_SAMPLE_FIELD_FRACTION : 0u) |
           (o->velocity ? (uint32_t)SPHX_SAMPLE_FIELD_VELOCITY : 0u) | (o->count ? (uint32_t)SPHX_SAMPLE_FIELD_COUNT : 0u);
}
// the argument rules both calls share, in the order of the single-context calls; nullptr: they pass
const char* sample_args_error(const sphx_multi* m, int kind, uint32_t flags, const sphx_multi_sample_out* out) {
    if (!out) return "out is NULL";
    if (!sample_fields(out)) return "out requests no output (density, fraction, velocity and count are NULL)";
    if (kind != SPHX_KERNEL_WENDLAND_C2 && kind != SPHX_KERNEL_POLY6 && kind != SPHX_KERNEL_SPIKY) return "unknown kernel_kind";
    if (flags) return "unknown flags bits (there is no device-pointer path across several devices)";
    if (m->world > 64) return "more than 64 tiles";
    if (m->rank_mode && !out->tile) return "out->tile is NULL in rank mode (it says which points this rank answered)";
    return nullptr;
}
// every requested array zero, tile -1: the answer for a point none of the local tiles owns
void sample_fill_absent(const sphx_multi_sample_out& o, size_t n) {
    if (o.density) std::memset(o.density, 0, n * 4);
    if (o.fraction) std::memset(o.fraction, 0, n * 4);
    if (o.velocity) std::memset(o.velocity, 0, 2 * n * 4);
    if (o.count) std::memset(o.count, 0, n * 4);
    if (o.tile) std::fill(o.tile, o.tile + n, (int32_t)-1);
}
// the ghost band (TileDriver::sample_band), every tile on its own host thread: a refresh meets the other tiles in the exchange
int sample_band(sphx_multi* m) { return m->each([](TileDriver& t, size_t) { return t.sample_band(); }); }
int sample_tile_failed(sphx_multi* m, size_t k, int rc) {
    m->err = "tile " + std::to_string(k) + ": " + m->tiles[k]->err;
    return rc;
}

}  // namespace

extern "C" {

int sphx_sample_merge(uint32_t n, const sphx_multi_sample_out* parts, uint32_t n_parts, const sphx_multi_sample_out* out) {
    auto bad = [](const char* what) {
        g_multi_error = std::string("sphx_sample_merge: ") + what;  // (no object to hang the message on: sphx_multi_last_error(NULL))
        return SPHX_ERR_INVALID_ARGUMENT;
    };
    if (!out) return bad("out is NULL");
    if (!sample_fields(out) && !out->tile) return bad("out requests no output (every pointer is NULL)");
    if (n_parts && !parts) return bad("parts is NULL with n_parts > 0");
    std::vector<sh::Part> ps(n_parts);
    for (uint32_t p = 0; p < n_parts; ++p) {
        const sphx_multi_sample_out& q = parts[p];
        if (!q.tile) return bad("a part has no tile array");
        if ((out->density && !q.density) || (out->fraction && !q.fraction) || (out->velocity && !q.velocity) || (out->count && !q.count))
            return bad("out asks for an array a part lacks");
        ps[p] = sh::Part{(const uint32_t*)q.density, (const uint32_t*)q.fraction, (const uint32_t*)q.velocity, q.count, q.tile};
    }
    sh::merge(n, ps.data(), n_parts, sh::Acc{(uint32_t*)out->density, (uint32_t*)out->fraction, (uint32_t*)out->velocity, out->count, out->tile});
    return SPHX_OK;
}

int sphx_multi_tile_rects(const sphx_multi* m, sphx_tile_rect* out, uint32_t* inout_n) {
    if (!m || !inout_n) return SPHX_ERR_INVALID_ARGUMENT;
    if (!m->uploaded) return SPHX_ERR_NOT_READY;  // (the layout is made from the uploaded particles)
    const auto rects = m->tiles[0]->layout.rects();
    const uint32_t cap = *inout_n;
    *inout_n = (uint32_t)rects.size();
    if (cap < rects.size()) return SPHX_ERR_CAPACITY;
    if (!out) return SPHX_ERR_INVALID_ARGUMENT;
    for (size_t k = 0; k < rects.size(); ++k) out[k] = sphx_tile_rect{rects[k].x0, rects[k].x1, rects[k].y0, rects[k].y1};
    return SPHX_OK;
}

int sphx_multi_ghost_rings(const sphx_multi* m, double* out3) {
    if (!m || !out3) return SPHX_ERR_INVALID_ARGUMENT;
    const TileDriver& t = *m->tiles[0];
    out3[0] = t.valid, out3[1] = t.kvalid, out3[2] = t.avalid;
    return SPHX_OK;
}

int sphx_multi_sample_points(sphx_multi* m, const float* xy, uint32_t n, int kernel_kind, uint32_t flags, const sphx_multi_sample_out* out) {
    if (!m) return SPHX_ERR_INVALID_ARGUMENT;
    const char* const fn = "sphx_multi_sample_points";
    if (const char* b = sample_args_error(m, kernel_kind, flags, out)) return sample_bad(m, fn, b);
    if (n && !xy) return sample_bad(m, fn, "xy is NULL with n > 0");
    if (n >= (1u << 31)) return sample_bad(m, fn, "n must be < 2^31");
    if (n == 0) return SPHX_OK;
    int rc;
    if ((rc = multi_state_ready(m, fn, true))) return rc;
    if ((rc = sample_band(m))) return rc;
    const uint32_t fields = sample_fields(out);
    // every local tile enqueues on its own stream and device first, then the records are collected: the tiles' passes overlap
    for (size_t k = 0; k < m->tiles.size(); ++k)
        if ((rc = m->tiles[k]->sample_points_enqueue(xy, n, kernel_kind, fields))) return sample_tile_failed(m, k, rc);
    sample_fill_absent(*out, n);
    if (m->sample_records.size() < 6 * (size_t)n) m->sample_records.resize(6 * (size_t)n);  // (a tile fills what it reports)
    uint32_t* const records = m->sample_records.data();
    for (size_t k = 0; k < m->tiles.size(); ++k) {
        uint32_t n_rec = 0;
        if ((rc = m->tiles[k]->sample_points_fetch(records, n, &n_rec))) return sample_tile_failed(m, k, rc);
        const int32_t rank = (int32_t)track_tile_rank(m, k);
        for (uint32_t r = 0; r < n_rec; ++r) {
            const uint32_t* const w = records + 6 * (size_t)r;
            const uint32_t i = w[0];
            if (i >= n) {
                m->err = std::string(fn) + ": tile " + std::to_string(k) + " returned a record outside the point set";
                return SPHX_ERR_HIP;
            }
            if (out->density) std::memcpy(out->density + i, w + 1, 4);
            if (out->fraction) std::memcpy(out->fraction + i, w + 2, 4);
            if (out->velocity) std::memcpy(out->velocity + 2 * (size_t)i, w + 3, 8);
            if (out->count) out->count[i] = w[5];
            if (out->tile) out->tile[i] = rank;
        }
    }
    return SPHX_OK;
}

int sphx_multi_sample_grid(sphx_multi* m, float x0, float y0, float dx, float dy, uint32_t nx, uint32_t ny, int kernel_kind, uint32_t flags,
                           const sphx_multi_sample_out* out) {
    if (!m) return SPHX_ERR_INVALID_ARGUMENT;
    const char* const fn = "sphx_multi_sample_grid";
    if (const char* b = sample_args_error(m, kernel_kind, flags, out)) return sample_bad(m, fn, b);
    if (!std::isfinite(x0) || !std::isfinite(y0)) return sample_bad(m, fn, "x0 / y0 must be finite");
    if (!std::isfinite(dx) || !(dx > 0.0f)) return sample_bad(m, fn, "dx must be finite and > 0");
    if (!std::isfinite(dy) || !(dy > 0.0f)) return sample_bad(m, fn, "dy must be finite and > 0");
    const uint64_t np = (uint64_t)nx * ny;
    if (np >= (1ull << 31)) return sample_bad(m, fn, "nx * ny must be < 2^31");
    if (np == 0) return SPHX_OK;
    int rc;
    if ((rc = multi_state_ready(m, fn, true))) return rc;
    if ((rc = sample_band(m))) return rc;
    const uint32_t fields = sample_fields(out);
    for (size_t k = 0; k < m->tiles.size(); ++k)
        if ((rc = m->tiles[k]->sample_window_enqueue(x0, y0, dx, dy, nx, ny, kernel_kind, fields))) return sample_tile_failed(m, k, rc);
    if (m->rank_mode) sample_fill_absent(*out, (size_t)np);  // (in-process the windows of the tiles cover the lattice)
    uint64_t covered = 0;
    for (size_t k = 0; k < m->tiles.size(); ++k) {
        TileDriver& t = *m->tiles[k];
        sphx_sample_out win;
        if ((rc = t.sample_window_fetch(fields, &win))) return sample_tile_failed(m, k, rc);
        const uint32_t ix0 = t.sample_win[0], wnx = t.sample_win[1] - t.sample_win[0], iy0 = t.sample_win[2], wny = t.sample_win[3] - t.sample_win[2];
        if (t.sample_win[1] > nx || t.sample_win[3] > ny) {
            m->err = std::string(fn) + ": tile " + std::to_string(k) + " returned a window outside the lattice";
            return SPHX_ERR_HIP;
        }
        covered += (uint64_t)wnx * wny;
        const int32_t rank = (int32_t)track_tile_rank(m, k);
        for (uint32_t r = 0; r < wny && wnx; ++r) {  // the window's rows into the full arrays
            const size_t src = (size_t)r * wnx, dst = (size_t)(iy0 + r) * nx + ix0;
            if (out->density) std::memcpy(out->density + dst, win.density + src, (size_t)wnx * 4);
            if (out->fraction) std::memcpy(out->fraction + dst, win.fraction + src, (size_t)wnx * 4);
            if (out->velocity) std::memcpy(out->velocity + 2 * dst, win.velocity + 2 * src, (size_t)wnx * 8);
            if (out->count) std::memcpy(out->count + dst, win.count + src, (size_t)wnx * 4);
            if (out->tile) std::fill(out->tile + dst, out->tile + dst + wnx, rank);
        }
    }
    if (!m->rank_mode && covered != np) {  // (the rectangles partition the cell domain: the windows partition the lattice)
        m->err = std::string(fn) + ": the tiles' windows do not cover the lattice";
        return SPHX_ERR_HIP;
    }
    return SPHX_OK;
}

}  // extern "C"

// ---- free surface of a tiled run (include/sphx.h, "free surface of a tiled run"; the device passes are csrc/sphx_contour.inc, the
// apron look-up and the merge csrc/sphx_contour_merge.hpp) --------------------------------------------------------------------------------
namespace {

namespace ch = sphx_contour_host;

int contour_tile_failed(sphx_multi* m, size_t k, const char* call, int rc) {
    m->tiles[k]->err = std::string(call) + ": " + sphx_last_error(m->tiles[k]->ctx);
    return sample_tile_failed(m, k, rc);
}

// The borders of all `world` tiles as one vector (ch::border_offsets).  In-process every entry was fetched.  Rank mode: this rank filled
// its own entries; each word crosses as (double)(bit pattern) with zeros from the other ranks, summed eight at a time — integers below
// 2^32, so the sum is the word (the trick of stats_gather).
int contour_share_borders(sphx_multi* m, std::vector<uint32_t>& borders) {
    if (!m->rank_mode) return SPHX_OK;
    TileDriver& t = *m->tiles[0];
    for (size_t at = 0; at < borders.size(); at += 8) {
        const int n = (int)std::min<size_t>(8, borders.size() - at);
        double in[8] = {0}, out[8] = {0};
        for (int k = 0; k < n; ++k) in[k] = (double)borders[at + k];
        const int rc = t.comm->allreduce(in, n, 0, out);
        if (rc) {
            m->err = "sphx_multi_surface_contour: the windows' borders could not be exchanged between the ranks";
            return t.fail(rc, m->err);
        }
        for (int k = 0; k < n; ++k) borders[at + k] = (uint32_t)out[k];
    }
    return SPHX_OK;
}

}  // namespace

extern "C" {

int sphx_contour_merge(const sphx_multi_contour_out* parts, const uint32_t* stored, uint32_t n_parts, uint32_t cap_segments,
                       const sphx_multi_contour_out* out) {
    auto bad = [](const char* what) {
        g_multi_error = std::string("sphx_contour_merge: ") + what;  // (no object to hang the message on: sphx_multi_last_error(NULL))
        return SPHX_ERR_INVALID_ARGUMENT;
    };
    if (!out) return bad("out is NULL");
    if (!out->count) return bad("out->count is NULL");
    if (n_parts && (!parts || !stored)) return bad("parts or stored is NULL with n_parts > 0");
    std::vector<ch::MergePart> ps(n_parts);
    uint64_t total = 0;
    bool truncated = false;
    for (uint32_t p = 0; p < n_parts; ++p) {
        const sphx_multi_contour_out& q = parts[p];
        if (!q.count) return bad("a part has no count");
        if (stored[p] > q.count[0]) return bad("a part stores more entries than its count");
        if (stored[p] && !q.cell) return bad("a part has no cell array (the merge orders by it)");
        if (stored[p] && ((out->segments && cap_segments && !q.segments) || (out->tile && cap_segments && !q.tile))) return bad("out asks for an array a part lacks");
        total += q.count[0];
        truncated = truncated || q.count[0] > stored[p];
        ps[p] = ch::MergePart{q.segments, q.cell, q.tile, -1, stored[p]};
    }
    if (total > 0xffffffffull) return bad("the parts' counts sum to 2^32 or more");
    out->count[0] = (uint32_t)total;
    if (truncated) {
        g_multi_error = "sphx_contour_merge: a part holds fewer entries than its count (call again with a capacity of at least the count)";
        return SPHX_ERR_CAPACITY;
    }
    ch::merge(ps.data(), n_parts, cap_segments, ch::MergeOut{out->segments, out->cell, out->tile});
    return SPHX_OK;
}

int sphx_multi_surface_contour(sphx_multi* m, float x0, float y0, float dx, float dy, uint32_t nx, uint32_t ny, int kernel_kind, int field, float iso,
                               uint32_t cap_segments, uint32_t flags, const sphx_multi_contour_out* out) {
    if (!m) return SPHX_ERR_INVALID_ARGUMENT;
    const char* const fn = "sphx_multi_surface_contour";
    if (!out) return sample_bad(m, fn, "out is NULL");
    if (!out->count) return sample_bad(m, fn, "out->count is NULL");
    if (kernel_kind != SPHX_KERNEL_WENDLAND_C2 && kernel_kind != SPHX_KERNEL_POLY6 && kernel_kind != SPHX_KERNEL_SPIKY) return sample_bad(m, fn, "unknown kernel_kind");
    if (field != SPHX_CONTOUR_FIELD_FRACTION && field != SPHX_CONTOUR_FIELD_DENSITY) return sample_bad(m, fn, "unknown field");
    if (flags) return sample_bad(m, fn, "unknown flags bits (there is no device-pointer path across several devices)");
    if (!std::isfinite(iso)) return sample_bad(m, fn, "iso must be finite");
    if (m->world > 64) return sample_bad(m, fn, "more than 64 tiles");
    if (m->rank_mode && cap_segments && !out->cell) return sample_bad(m, fn, "out->cell is NULL in rank mode (sphx_contour_merge orders the parts by it)");
    if (!std::isfinite(x0) || !std::isfinite(y0)) return sample_bad(m, fn, "x0 / y0 must be finite");
    if (!std::isfinite(dx) || !(dx > 0.0f)) return sample_bad(m, fn, "dx must be finite and > 0");
    if (!std::isfinite(dy) || !(dy > 0.0f)) return sample_bad(m, fn, "dy must be finite and > 0");
    if ((uint64_t)nx * ny >= (1ull << 31)) return sample_bad(m, fn, "nx * ny must be < 2^31");
    if (nx < 2u || ny < 2u) {  // no cell (this covers nx * ny == 0)
        out->count[0] = 0u;
        return SPHX_OK;
    }
    int rc;
    if ((rc = multi_state_ready(m, fn, true))) return rc;
    if ((rc = sample_band(m))) return rc;
    // every tile's window, on every rank by the same bisection over the layout's rectangles
    const uint32_t world = (uint32_t)m->world;
    const TileDriver& t0 = *m->tiles[0];
    const auto rects = t0.layout.rects();
    if (rects.size() != world) {
        m->err = std::string(fn) + ": the layout does not name one rectangle per tile";
        return SPHX_ERR_HIP;
    }
    std::vector<sh::Window> wins(world);
    for (uint32_t g = 0; g < world; ++g)
        wins[g] = sh::lattice_window(x0, y0, dx, dy, nx, ny, t0.grid_min[0], t0.grid_min[1], t0.cell_inv, rects[g].x0, rects[g].x1, rects[g].y0, rects[g].y1);
    if (!ch::windows_cover(wins.data(), world, nx, ny)) {
        m->err = std::string(fn) + ": the tiles' windows do not cover the lattice";
        return SPHX_ERR_HIP;
    }
    const std::vector<size_t> off = ch::border_offsets(wins.data(), world);
    const size_t n_local = m->tiles.size();
    // 1. every local tile samples its padded window and packs its border, on its own stream and device
    for (size_t k = 0; k < n_local; ++k) {
        uint32_t win[4];
        if ((rc = sphx_tile_contour_sample(m->tiles[k]->ctx, x0, y0, dx, dy, nx, ny, kernel_kind, field, win)))
            return contour_tile_failed(m, k, "sphx_tile_contour_sample", rc);
        const sh::Window& w = wins[track_tile_rank(m, k)];
        if (win[0] != w.ix0 || win[1] != w.ix1 || win[2] != w.iy0 || win[3] != w.iy1) {
            m->err = std::string(fn) + ": tile " + std::to_string(k) + " reports another window than its rectangle gives";
            return SPHX_ERR_HIP;
        }
    }
    // 2. the borders come back (one small copy and one wait per tile) and cross the ranks
    std::vector<uint32_t> borders(off[world], 0u);
    for (size_t k = 0; k < n_local; ++k) {
        const uint32_t g = track_tile_rank(m, k);
        if ((rc = sphx_tile_contour_border_fetch(m->tiles[k]->ctx, borders.data() + off[g], (uint32_t)(off[g + 1] - off[g]))))
            return contour_tile_failed(m, k, "sphx_tile_contour_border_fetch", rc);
    }
    if ((rc = contour_share_borders(m, borders))) return rc;
    // 3. every local tile gets its apron by node look-up and enqueues the cut (the aprons live until the parts are fetched)
    std::vector<std::vector<uint32_t>> aprons(n_local);
    std::vector<uint32_t> caps(n_local, 0u);
    std::vector<size_t> idx;
    for (size_t k = 0; k < n_local; ++k) {
        const uint32_t g = track_tile_rank(m, k);
        uint32_t bad_ix = 0, bad_iy = 0;
        if (ch::apron_indices(wins.data(), off.data(), world, nx, ny, g, idx, &bad_ix, &bad_iy)) {
            m->err = std::string(fn) + ": apron node (" + std::to_string(bad_ix) + ", " + std::to_string(bad_iy) + ") of tile " + std::to_string(g) +
                     " is not in exactly one window's first row or column";
            return SPHX_ERR_HIP;
        }
        aprons[k].resize(idx.size());
        for (size_t i = 0; i < idx.size(); ++i) aprons[k][i] = borders[idx[i]];
        caps[k] = (uint32_t)std::min<uint64_t>(cap_segments, 2ull * ch::window_cells(wins[g], nx, ny));
        if ((rc = sphx_tile_contour_cut(m->tiles[k]->ctx, iso, caps[k], aprons[k].data(), (uint32_t)aprons[k].size())))
            return contour_tile_failed(m, k, "sphx_tile_contour_cut", rc);
    }
    // 4. the parts: rank mode writes this rank's straight into out; in-process they are merged by cell word
    if (m->rank_mode) {
        uint32_t count = 0;
        if ((rc = sphx_tile_contour_fetch(m->tiles[0]->ctx, out->segments, out->cell, &count))) return contour_tile_failed(m, 0, "sphx_tile_contour_fetch", rc);
        out->count[0] = count;
        const uint32_t got = std::min(count, caps[0]);
        if (out->tile) std::fill(out->tile, out->tile + got, (int32_t)track_tile_rank(m, 0));
        return SPHX_OK;
    }
    std::vector<std::vector<uint32_t>> cells(n_local);
    std::vector<std::vector<float>> segs(n_local);
    std::vector<ch::MergePart> parts(n_local);
    uint64_t total = 0;
    for (size_t k = 0; k < n_local; ++k) {
        cells[k].resize(caps[k]);
        if (out->segments) segs[k].resize(4 * (size_t)caps[k]);
        uint32_t count = 0;
        if ((rc = sphx_tile_contour_fetch(m->tiles[k]->ctx, out->segments && caps[k] ? segs[k].data() : nullptr, caps[k] ? cells[k].data() : nullptr, &count)))
            return contour_tile_failed(m, k, "sphx_tile_contour_fetch", rc);
        total += count;
        parts[k] = ch::MergePart{out->segments ? segs[k].data() : nullptr, cells[k].data(), nullptr, (int32_t)k, std::min(count, caps[k])};
    }
    out->count[0] = (uint32_t)total;  // (2 * cells < 2^32)
    ch::merge(parts.data(), (uint32_t)n_local, cap_segments, ch::MergeOut{out->segments, out->cell, out->tile});
    return SPHX_OK;
}

}  // extern "C"

// ---- per-particle flow fields of a tiled run (include/sphx.h, "per-particle flow fields of a tiled run"; the device passes are
// csrc/sphx_fields.inc) -------------------------------------------------------------------------------------------------------------------
extern "C" {

int sphx_multi_particle_fields(sphx_multi* m, uint32_t flags, const sphx_multi_fields_out* out, uint64_t* inout_n) {
    if (!m) return SPHX_ERR_INVALID_ARGUMENT;
    const char* const fn = "sphx_multi_particle_fields";
    if (!out) return sample_bad(m, fn, "out is NULL");
    if (!inout_n) return sample_bad(m, fn, "inout_n is NULL");
    const uint32_t mask = (out->vel_grad ? (uint32_t)SPHX_FIELD_VEL_GRAD : 0u) | (out->divergence ? (uint32_t)SPHX_FIELD_DIVERGENCE : 0u) |
                          (out->vorticity ? (uint32_t)SPHX_FIELD_VORTICITY : 0u) | (out->color_grad ? (uint32_t)SPHX_FIELD_COLOR_GRAD : 0u);
    if (!mask) return sample_bad(m, fn, "out requests no output (vel_grad, divergence, vorticity and color_grad are NULL)");
    if (flags) return sample_bad(m, fn, "unknown flags bits (there is no device-pointer path across several devices)");
    int rc;
    if ((rc = multi_state_ready(m, fn, true))) return rc;
    if ((rc = sample_band(m))) return rc;
    // the capacity, before any walk: every tile counts what it owns on its device (the host's count lags a migration)
    std::vector<uint32_t> owned(m->tiles.size(), 0u);
    uint64_t total = 0;
    for (size_t k = 0; k < m->tiles.size(); ++k) {
        if ((rc = sphx_tile_owned_count(m->tiles[k]->ctx, &owned[k]))) {
            m->tiles[k]->err = std::string("sphx_tile_owned_count: ") + sphx_last_error(m->tiles[k]->ctx);
            return sample_tile_failed(m, k, rc);
        }
        total += owned[k];
    }
    const uint64_t cap = *inout_n;
    *inout_n = total;
    if (cap < total) {
        m->err = std::string(fn) + ": *inout_n is smaller than the " + std::to_string(total) + " particles the local tiles own";
        return SPHX_ERR_CAPACITY;
    }
    if (!total) return SPHX_OK;
    // every local tile enqueues on its own stream and device first, then the parts are collected: the tiles' passes overlap
    for (size_t k = 0; k < m->tiles.size(); ++k)
        if (owned[k] && (rc = sphx_tile_particle_fields_enqueue(m->tiles[k]->ctx, mask, out->ids ? 1u : 0u))) {
            m->tiles[k]->err = std::string("sphx_tile_particle_fields_enqueue: ") + sphx_last_error(m->tiles[k]->ctx);
            return sample_tile_failed(m, k, rc);
        }
    uint64_t at = 0;
    for (size_t k = 0; k < m->tiles.size(); ++k) {
        if (!owned[k]) continue;
        const sphx_fields_out part{out->vel_grad ? out->vel_grad + 4 * at : nullptr, out->divergence ? out->divergence + at : nullptr,
                                   out->vorticity ? out->vorticity + at : nullptr, out->color_grad ? out->color_grad + 2 * at : nullptr};
        uint32_t got = 0;
        if ((rc = sphx_tile_particle_fields_fetch(m->tiles[k]->ctx, &part, out->ids ? out->ids + at : nullptr, owned[k], &got))) {
            m->tiles[k]->err = std::string("sphx_tile_particle_fields_fetch: ") + sphx_last_error(m->tiles[k]->ctx);
            return sample_tile_failed(m, k, rc);
        }
        if (got != owned[k]) {
            m->err = std::string(fn) + ": tile " + std::to_string(k) + " answered another number of particles than it counted";
            return SPHX_ERR_HIP;
        }
        if (out->tile) std::fill(out->tile + at, out->tile + at + got, (int32_t)track_tile_rank(m, k));
        at += got;
    }
    return SPHX_OK;
}

}  // extern "C"

// ---- neighbour queries of a tiled run (include/sphx.h, "neighbour queries of a tiled run"; the device passes are csrc/sphx_query.inc,
// the fold csrc/sphx_query_merge.hpp) --------------------------------------------------------------------------------------------------
namespace {

namespace qh = sphx_query_host;
static_assert(qh::ERR_CAPACITY == SPHX_ERR_CAPACITY && qh::OK == SPHX_OK && qh::NONE == SPHX_QUERY_NONE, "the fold's codes are the header's");

qh::Out query_out(const sphx_multi_query_out& o, uint64_t cap) {
    qh::Out r;
    r.offsets = o.offsets;
    r.id = o.id;
    r.d2 = (uint32_t*)o.dist_sq;
    r.slot = o.slot;
    r.nearest_id = o.nearest_id;
    r.nearest_slot = o.nearest_slot;
    r.nearest_d2 = (uint32_t*)o.nearest_dist_sq;
    r.tile = o.tile;
    r.count = o.count;
    r.cap = cap;
    return r;
}

}  // namespace

extern "C" {

int sphx_query_merge(uint32_t m, const sphx_multi_query_out* parts, const uint64_t* parts_cap, uint32_t n_parts, uint64_t cap_entries,
                     const sphx_multi_query_out* out) {
    auto bad = [](const char* what) {
        g_multi_error = std::string("sphx_query_merge: ") + what;  // (no object to hang the message on: sphx_multi_last_error(NULL))
        return SPHX_ERR_INVALID_ARGUMENT;
    };
    if (!out) return bad("out is NULL");
    if (!out->count) return bad("out->count is NULL");
    if (n_parts && !parts) return bad("parts is NULL with n_parts > 0");
    if (m >= (1u << 31)) return bad("m must be < 2^31");
    const bool lists = out->id || out->dist_sq || out->slot;
    if (n_parts && lists && !parts_cap) return bad("parts_cap is NULL while out asks for entries");
    std::vector<qh::Part> ps(n_parts);
    for (uint32_t p = 0; p < n_parts; ++p) {
        const sphx_multi_query_out& q = parts[p];
        if (!q.offsets) return bad("a part has no offsets array");
        if (!q.tile) return bad("a part has no tile array");
        if ((out->id && !q.id) || (out->dist_sq && !q.dist_sq) || (out->slot && !q.slot) || (out->nearest_id && !q.nearest_id) ||
            (out->nearest_slot && !q.nearest_slot) || (out->nearest_dist_sq && !q.nearest_dist_sq))
            return bad("out asks for an array a part lacks");
        qh::Part& r = ps[p];
        r.n = m;
        r.offset = q.offsets;
        r.total = q.offsets[m];
        r.tile = q.tile;
        r.nearest_id = q.nearest_id;
        r.nearest_slot = q.nearest_slot;
        r.nearest_d2 = (const uint32_t*)q.nearest_dist_sq;
        r.id = q.id;
        r.d2 = (const uint32_t*)q.dist_sq;
        r.slot = q.slot;
        r.held = parts_cap ? std::min<uint64_t>(q.offsets[m], parts_cap[p]) : 0u;
    }
    const int rc = qh::merge(m, ps.data(), n_parts, query_out(*out, cap_entries));
    if (rc) g_multi_error = "sphx_query_merge: the result needs an entry that a part truncated (its parts_cap is below its count)";
    return rc;
}

int sphx_multi_query_radius(sphx_multi* m, const float* xy, uint32_t n, float radius, uint64_t cap_entries, uint32_t flags, const sphx_multi_query_out* out) {
    if (!m) return SPHX_ERR_INVALID_ARGUMENT;
    const char* const fn = "sphx_multi_query_radius";
    if (!out) return sample_bad(m, fn, "out is NULL");
    if (!out->count) return sample_bad(m, fn, "out->count is NULL");
    if (n && !xy) return sample_bad(m, fn, "xy is NULL with m > 0");
    if (flags & ~(uint32_t)SPHX_QUERY_BOUNDARY) return sample_bad(m, fn, "unknown flags bits (there is no device-pointer path across several devices)");
    if (n >= (1u << 31)) return sample_bad(m, fn, "m must be < 2^31");
    if (!std::isfinite(radius) || !(radius > 0.0f) || radius > m->P.smoothing_length)
        return sample_bad(m, fn, "radius must be finite, > 0 and <= smoothing_length");
    if (m->world > 64) return sample_bad(m, fn, "more than 64 tiles");
    if (m->rank_mode && !out->tile) return sample_bad(m, fn, "out->tile is NULL in rank mode (it says which points this rank answered)");
    if (n == 0) {
        out->count[0] = 0u;
        if (out->offsets) out->offsets[0] = 0u;
        return SPHX_OK;
    }
    int rc;
    if ((rc = multi_state_ready(m, fn, true))) return rc;
    const bool lists = out->id || out->dist_sq || out->slot;
    const bool nearest = out->nearest_id || out->nearest_slot || out->nearest_dist_sq;
    const uint64_t cap = lists ? cap_entries : 0u;
    // every local tile enqueues on its own stream and device first; then the totals are read and the emitting walks enqueued; then the
    // parts are collected: the tiles' passes overlap.  No tile exchanges anything (TileDriver::query_enqueue).
    for (size_t k = 0; k < m->tiles.size(); ++k)
        if ((rc = m->tiles[k]->query_enqueue(xy, n, radius, flags, nearest))) return sample_tile_failed(m, k, rc);
    for (size_t k = 0; k < m->tiles.size(); ++k)
        if ((rc = m->tiles[k]->query_size(cap))) return sample_tile_failed(m, k, rc);
    std::vector<qh::Part> ps(m->tiles.size());
    for (size_t k = 0; k < m->tiles.size(); ++k) {
        TileDriver& t = *m->tiles[k];
        if ((rc = t.query_fetch(cap, nearest, lists))) return sample_tile_failed(m, k, rc);
        const sphx_tile_query_part& q = t.query_part;
        qh::Part& r = ps[k];
        r.point = q.point;
        r.n = q.n_points;
        r.offset = q.offset;
        r.total = q.total;
        r.rank = (int32_t)track_tile_rank(m, k);
        r.nearest_id = q.nearest_id;
        r.nearest_slot = q.nearest_slot;
        r.nearest_d2 = (const uint32_t*)q.nearest_dist_sq;
        r.id = q.id;
        r.d2 = (const uint32_t*)q.dist_sq;
        r.slot = q.slot;
        r.held = lists ? q.kept : 0u;
        if (flags & SPHX_QUERY_BOUNDARY) r.id_map = t.clip_map.data(), r.id_map_n = (uint32_t)t.clip_map.size();
        for (uint32_t j = 0; j < q.n_points; ++j)
            if (q.point[j] >= n || (j && q.point[j] <= q.point[j - 1])) {
                m->err = std::string(fn) + ": tile " + std::to_string(k) + " returned a record outside the point set";
                return SPHX_ERR_HIP;
            }
    }
    if ((rc = qh::merge(n, ps.data(), (uint32_t)ps.size(), query_out(*out, cap)))) {
        m->err = std::string(fn) + ": a tile kept fewer entries than the merged list needs";
        return rc;
    }
    return SPHX_OK;
}

int sphx_multi_select(sphx_multi* m, const sphx_rect* rects, uint32_t n_rects, uint32_t flags, uint64_t cap, const sphx_multi_select_out* out) {
    if (!m) return SPHX_ERR_INVALID_ARGUMENT;
    const char* const fn = "sphx_multi_select";
    if (!out) return sample_bad(m, fn, "out is NULL");
    if (!out->count) return sample_bad(m, fn, "out->count is NULL");
    if (n_rects > SPHX_REMOVE_MAX_RECTS) return sample_bad(m, fn, "n_rects is larger than SPHX_REMOVE_MAX_RECTS");
    if (n_rects && !rects) return sample_bad(m, fn, "rects is NULL with n_rects > 0");
    if (flags & ~(uint32_t)SPHX_SELECT_OUTSIDE) return sample_bad(m, fn, "unknown flags bits (there is no device-pointer path across several devices)");
    for (uint32_t k = 0; k < n_rects; ++k)
        if (std::isnan(rects[k].x0) || std::isnan(rects[k].y0) || std::isnan(rects[k].x1) || std::isnan(rects[k].y1))
            return sample_bad(m, fn, "a rectangle bound is NaN (rects)");
    if (m->world > 64) return sample_bad(m, fn, "more than 64 tiles");
    int rc;
    if ((rc = multi_state_ready(m, fn, true))) return rc;
    for (size_t k = 0; k < m->tiles.size(); ++k)
        if ((rc = m->tiles[k]->select_enqueue(rects, n_rects, flags))) return sample_tile_failed(m, k, rc);
    std::vector<uint32_t> totals(m->tiles.size(), 0u);
    for (size_t k = 0; k < m->tiles.size(); ++k)
        if ((rc = m->tiles[k]->select_fetch(0u, &totals[k]))) return sample_tile_failed(m, k, rc);
    const bool lists = out->id || out->tile || out->slot;
    uint64_t at = 0;
    for (size_t k = 0; k < m->tiles.size(); ++k) {
        const uint32_t got = (lists && at < cap) ? (uint32_t)std::min<uint64_t>(totals[k], cap - at) : 0u;
        if (got) {
            TileDriver& t = *m->tiles[k];
            if (out->id || out->slot) {
                uint32_t again = 0;
                if ((rc = t.select_fetch(got, &again))) return sample_tile_failed(m, k, rc);
                if (out->slot) std::memcpy(out->slot + at, t.select_host.data(), (size_t)got * 4);
                if (out->id) std::memcpy(out->id + at, t.select_host.data() + got, (size_t)got * 4);
            }
            if (out->tile) std::fill(out->tile + at, out->tile + at + got, (int32_t)track_tile_rank(m, k));
        }
        at += totals[k];
    }
    out->count[0] = at;
    return SPHX_OK;
}

}  // extern "C"

// ---- gauges and probes of a tiled run (include/sphx.h, "gauges and probes of a tiled run"; the device passes are csrc/sphx_gauge.inc, the
// intervals csrc/sphx_gauge_window.hpp, the fold csrc/sphx_gauge_merge.hpp) ---------------------------------------------------------------
namespace {

namespace gh = sphx_gauge_host;

// the argument rules of sphx_gauge_levels that need no context, in its order; nullptr: they pass
const char* gauge_args_error(const sphx_gauge* gauges, uint32_t n_gauges, int kind, int field, float iso, uint64_t* total) {
    if (const char* bad = gh::check(gauges, n_gauges, iso, total)) return bad;
    if (kind != SPHX_KERNEL_WENDLAND_C2 && kind != SPHX_KERNEL_POLY6 && kind != SPHX_KERNEL_SPIKY) return "unknown kernel_kind";
    if (field != SPHX_GAUGE_FIELD_FRACTION && field != SPHX_GAUGE_FIELD_DENSITY) return "unknown field";
    return nullptr;
}

bool probe_installed(const sphx_multi* m) { return m->probe.epoch != 0 && m->tiles[0]->probe_epoch == m->probe.epoch; }

}  // namespace

extern "C" {

int sphx_gauge_merge(const sphx_gauge* gauges, uint32_t n_gauges, float iso, const sphx_gauge_part* parts, uint32_t n_parts, sphx_gauge_rec* out) {
    auto bad = [](const char* what) {
        g_multi_error = std::string("sphx_gauge_merge: ") + what;  // (no object to hang the message on: sphx_multi_last_error(NULL))
        return SPHX_ERR_INVALID_ARGUMENT;
    };
    if (!out) return bad("out is NULL");
    uint64_t total;
    if (const char* b = gh::check(gauges, n_gauges, iso, &total)) return bad(b);
    if (n_gauges && n_parts && !parts) return bad("parts is NULL with n_parts > 0");
    if (const char* b = gh::merge(gauges, n_gauges, iso, parts, n_parts, out)) return bad(b);
    return SPHX_OK;
}

int sphx_multi_gauge_levels(sphx_multi* m, const sphx_gauge* gauges, uint32_t n_gauges, int kernel_kind, int field, float iso, uint32_t flags,
                            sphx_gauge_rec* out, float* values, sphx_gauge_part* out_parts) {
    if (!m) return SPHX_ERR_INVALID_ARGUMENT;
    const char* const fn = "sphx_multi_gauge_levels";
    if (!out && !m->rank_mode) return sample_bad(m, fn, "out is NULL");
    uint64_t total = 0;
    if (const char* b = gauge_args_error(gauges, n_gauges, kernel_kind, field, iso, &total)) return sample_bad(m, fn, b);
    if (flags) return sample_bad(m, fn, "unknown flags bits (there is no device-pointer path across several devices)");
    if (m->world > 64) return sample_bad(m, fn, "more than 64 tiles");
    if (m->rank_mode && !out_parts) return sample_bad(m, fn, "out_parts is NULL in rank mode (the ranks' parts are folded with sphx_gauge_merge)");
    if (n_gauges == 0) return SPHX_OK;
    int rc;
    if ((rc = multi_state_ready(m, fn, true))) return rc;
    if ((rc = sample_band(m))) return rc;
    // every local tile enqueues on its own stream and device first, then the parts are collected: the tiles' passes overlap
    const size_t nt = m->tiles.size();
    for (size_t k = 0; k < nt; ++k)
        if ((rc = m->tiles[k]->gauge_enqueue(gauges, n_gauges, kernel_kind, field, iso))) return sample_tile_failed(m, k, rc);
    std::vector<sphx_gauge_part> parts(nt * n_gauges);
    for (size_t k = 0; k < nt; ++k) {
        TileDriver& t = *m->tiles[k];
        if ((rc = t.gauge_fetch(parts.data() + k * n_gauges, n_gauges, total, values != nullptr))) return sample_tile_failed(m, k, rc);
        if (values) {  // the tile's compact values to offset(g) + lo
            size_t at = 0, from = 0;
            for (uint32_t g = 0; g < n_gauges; ++g) {
                const uint32_t lo = t.gauge_lo_count[2 * (size_t)g], cnt = t.gauge_lo_count[2 * (size_t)g + 1];
                if (cnt) std::memcpy(values + at + lo, t.gauge_values.data() + from, (size_t)cnt * 4);
                from += cnt;
                at += gauges[g].n;
            }
        }
    }
    if (!m->rank_mode) {
        std::vector<gh::Words> rec(n_gauges);
        for (uint32_t g = 0; g < n_gauges; ++g)
            if (const char* b = gh::fold(gauges[g], iso, parts.data() + g, (uint32_t)nt, n_gauges, &rec[g])) {
                m->err = std::string(fn) + ": gauge " + std::to_string(g) + ": " + b;
                return SPHX_ERR_HIP;
            }
        std::memcpy(out, rec.data(), (size_t)n_gauges * sizeof(gh::Words));
    }
    if (out_parts) std::memcpy(out_parts, parts.data(), parts.size() * sizeof(sphx_gauge_part));
    return SPHX_OK;
}

int sphx_multi_probe_record(sphx_multi* m, const float* points_xy, uint32_t m_points, const sphx_gauge* gauges, uint32_t n_gauges, int kernel_kind,
                            int field, float iso, uint32_t max_frames, uint32_t every) {
    if (!m) return SPHX_ERR_INVALID_ARGUMENT;
    const char* const fn = "sphx_multi_probe_record";
    int rc;
    if ((rc = multi_state_ready(m, fn, false))) return rc;
    if (max_frames) {  // (checked before any tile is touched: all tiles keep the old recording or all get the new one)
        if (every == 0) return sample_bad(m, fn, "every must be >= 1");
        if (m_points >= (1u << 20)) return sample_bad(m, fn, "m_points must be < 2^20");
        if (m_points && !points_xy) return sample_bad(m, fn, "points_xy is NULL with m_points > 0");
        uint64_t total;
        if (const char* b = gauge_args_error(gauges, n_gauges, kernel_kind, field, iso, &total)) return sample_bad(m, fn, b);
        if (m_points + n_gauges == 0) return sample_bad(m, fn, "m_points + n_gauges is 0: nothing to record");
        if ((uint64_t)max_frames * (m_points + n_gauges) * 32ull > (64ull << 20)) {
            m->err = std::string(fn) + ": max_frames * (m_points + n_gauges) records exceed 64 MiB per tile";
            return SPHX_ERR_CAPACITY;
        }
    }
    MultiProbe& q = m->probe;
    q.on = max_frames != 0;
    q.points.assign(q.on && m_points ? points_xy : nullptr, q.on && m_points ? points_xy + 2 * (size_t)m_points : nullptr);
    q.gauges.assign(q.on && n_gauges ? gauges : nullptr, q.on && n_gauges ? gauges + n_gauges : nullptr);
    q.kind = kernel_kind, q.field = field, q.iso = iso;
    q.max_frames = max_frames;
    q.every = every ? every : 1u;
    q.epoch += 1;
    if (!m->uploaded) return SPHX_OK;  // (the contexts become tiles with the first upload: they install in front of their first frame)
    for (size_t k = 0; k < m->tiles.size(); ++k)
        if ((rc = m->tiles[k]->probe_install())) {
            m->err = "tile " + std::to_string(k) + ": " + m->tiles[k]->err;
            q.on = false;  // no half-made recording
            q.epoch += 1;
            for (auto& t : m->tiles) t->probe_install();
            return rc;
        }
    return SPHX_OK;
}

// (every tile counts the same steps and stores the same number of frames: the first local tile speaks for all)
int sphx_multi_probe_get_status(const sphx_multi* m, sphx_probe_status* out) {
    if (!m || !out) return SPHX_ERR_INVALID_ARGUMENT;
    if (probe_installed(m)) return sphx_probe_get_status(m->tiles[0]->ctx, out);
    std::memset(out, 0, sizeof(*out));
    const MultiProbe& q = m->probe;
    if (!q.on) return SPHX_OK;
    out->m_points = (uint32_t)(q.points.size() / 2);
    out->n_gauges = (uint32_t)q.gauges.size();
    out->recording = 1u;
    out->max_frames = q.max_frames;
    out->every = q.every;
    return SPHX_OK;
}

int sphx_multi_probe_read(sphx_multi* m, uint32_t first_frame, uint32_t n_frames, sphx_probe_rec* points_out, int32_t* point_tile,
                          sphx_gauge_rec* gauges_out, sphx_stats_frame* info) {
    if (!m) return SPHX_ERR_INVALID_ARGUMENT;
    const char* const fn = "sphx_multi_probe_read";
    int rc;
    if ((rc = multi_state_ready(m, fn, false))) return rc;
    sphx_probe_status st;
    sphx_multi_probe_get_status(m, &st);
    if ((uint64_t)first_frame + n_frames > st.frames)
        return sample_bad(m, fn, "first_frame + n_frames is beyond the frames recorded (sphx_multi_probe_get_status)");
    if (n_frames == 0) return SPHX_OK;
    if (m->world > 64) return sample_bad(m, fn, "more than 64 tiles");
    if (m->rank_mode && gauges_out && st.n_gauges)
        return sample_bad(m, fn, "gauges_out in rank mode (a rank holds parts: sphx_tile_probe_read, folded with sphx_gauge_merge)");
    const size_t nt = m->tiles.size(), np = (size_t)n_frames * st.m_points, ng = (size_t)n_frames * st.n_gauges;
    const bool want_points = (points_out || point_tile) && st.m_points, want_gauges = gauges_out && st.n_gauges;
    std::vector<sphx_probe_rec> pts(want_points ? nt * np : 0);
    std::vector<sphx_gauge_part> parts(want_gauges ? nt * ng : 0);
    for (size_t k = 0; k < nt; ++k)
        if ((rc = sphx_tile_probe_read(m->tiles[k]->ctx, first_frame, n_frames, want_points ? pts.data() + k * np : nullptr,
                                       want_gauges ? parts.data() + k * ng : nullptr, k == 0 ? info : nullptr))) {
            m->err = "tile " + std::to_string(k) + ": " + sphx_last_error(m->tiles[k]->ctx);
            return rc;
        }
    if (want_points) {
        std::vector<const sphx_probe_rec*> src(nt);
        std::vector<int32_t> tile_of(nt);
        for (size_t k = 0; k < nt; ++k) tile_of[k] = (int32_t)track_tile_rank(m, k);
        for (uint32_t f = 0; f < n_frames; ++f) {
            for (size_t k = 0; k < nt; ++k) src[k] = pts.data() + k * np + (size_t)f * st.m_points;
            gh::fold_points(st.m_points, src.data(), tile_of.data(), (uint32_t)nt, points_out ? points_out + (size_t)f * st.m_points : nullptr,
                            point_tile ? point_tile + (size_t)f * st.m_points : nullptr);
        }
    }
    if (want_gauges) {
        const MultiProbe& q = m->probe;
        std::vector<gh::Words> rec(ng);
        for (uint32_t f = 0; f < n_frames; ++f)
            for (uint32_t g = 0; g < st.n_gauges; ++g)
                if (const char* b = gh::fold(q.gauges[g], q.iso, parts.data() + (size_t)f * st.n_gauges + g, (uint32_t)nt, ng, &rec[(size_t)f * st.n_gauges + g])) {
                    m->err = std::string(fn) + ": frame " + std::to_string(first_frame + f) + ", gauge " + std::to_string(g) + ": " + b;
                    return SPHX_ERR_HIP;
                }
        std::memcpy(gauges_out, rec.data(), ng * sizeof(gh::Words));
    }
    return SPHX_OK;
}

}  // extern "C"
