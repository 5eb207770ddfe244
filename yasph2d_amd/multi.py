"""ctypes view of sphx_multi — the multi-GPU solver INSIDE libsphx (include/sphx.h, csrc/sphx_tiles.cpp).

`MultiSolver(devices=[...])` holds all tiles in this process (what a Rust host gets behind its one `Box<dyn Solver>`);
`MultiSolver.rank(...)` is ONE tile of a one-process-per-GPU run: with `dist=None` the library exchanges the halo records itself
(grouped ncclSend/ncclRecv over RCCL, shared-memory scalars), with a `torch.distributed` module the exchange is handed to it through
the sphx_comm_ops function table (the functional tests run that over gloo on a one-GPU box, where RCCL refuses two ranks per GPU).
The step loop is not here: it is C++ inside the library.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import SphxError, SphxMultiInfo, SphxMultiOptions, SphxStepStats

SAMPLE_FIELDS = ("density", "fraction", "velocity", "count")  # (yasph2d_amd.SAMPLE_FIELDS: the package imports this module lazily)


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


class TorchCommOps:
    """sphx_comm_ops over torch.distributed: halo records via batch_isend_irecv (nccl = RCCL: device buffers as they are; gloo:
    staged through the host), scalars via all_reduce (or the library's shared-memory reduction when `shm_name` is given)."""

    def __init__(self, dist, device, shm_name=None):
        import torch

        self.torch, self.dist, self.device = torch, dist, device
        self.rank, self.world = dist.get_rank(), dist.get_world_size()
        self.L = _lib.lib()
        self.shm = None
        if shm_name is not None:
            self.shm = self.L.sphx_shm_open(str(shm_name).encode(), self.rank, self.world)  # collective: returns when all ranks have joined
            if not self.shm:
                raise RuntimeError("sphx_shm_open failed")
        self._ex = _lib.COMM_EXCHANGE(self._exchange)
        self._ar = _lib.COMM_ALLREDUCE(self._allreduce)
        self._ab = _lib.COMM_ABORT(self._abort)
        self.ops = _lib.SphxCommOps(None, self.rank, self.world, self._ex, self._ar, self._ab)
        self.error = None

    def _tensor(self, ptr, nbytes):
        # a uint8 view of a device buffer libsphx owns (no copy): __cuda_array_interface__ v2
        holder = type("DevBuf", (), {"__cuda_array_interface__": {"shape": (nbytes,), "typestr": "|u1", "data": (int(ptr), False), "version": 2}})()
        return self.torch.as_tensor(holder, device=self.device)

    def _exchange(self, user, peers, n_peers, d_send, d_recv, nbytes, hip_stream):
        try:
            torch, dist = self.torch, self.dist
            stream = torch.cuda.ExternalStream(int(hip_stream), device=self.device)
            with torch.cuda.stream(stream):
                sends = [self._tensor(d_send[k], nbytes) for k in range(n_peers)]
                recvs = [self._tensor(d_recv[k], nbytes) for k in range(n_peers)]
                stage = dist.get_backend() == "gloo"
                if stage:
                    stream.synchronize()
                ss = [t.cpu() for t in sends] if stage else sends
                rs = [torch.empty_like(t) for t in ss] if stage else recvs
                ops = []
                for k in range(n_peers):
                    ops += [dist.P2POp(dist.isend, ss[k], int(peers[k])), dist.P2POp(dist.irecv, rs[k], int(peers[k]))]
                for w in dist.batch_isend_irecv(ops):
                    w.wait()
                if stage:
                    for k in range(n_peers):
                        recvs[k].copy_(rs[k])
            return 0
        except BaseException as e:  # noqa: BLE001 - must not unwind through the C frame
            self.error = e
            return _lib.ERR_HIP

    def _allreduce(self, user, pin, n, op, pout):
        try:
            if self.shm:
                return self.L.sphx_shm_allreduce(self.shm, C.cast(pin, C.c_void_p), n, op, C.cast(pout, C.c_void_p))
            torch, dist = self.torch, self.dist
            dev = torch.device("cpu") if dist.get_backend() == "gloo" else self.device
            t = torch.tensor([pin[k] for k in range(n)], dtype=torch.float64, device=dev)
            dist.all_reduce(t, op=dist.ReduceOp.MAX if op == 1 else dist.ReduceOp.SUM)
            for k, v in enumerate(t.tolist()):
                pout[k] = v
            return 0
        except BaseException as e:  # noqa: BLE001
            self.error = e
            return _lib.ERR_HIP

    def _abort(self, user):
        if self.shm:  # (torch.distributed has no abort: its collectives run into their own time-out)
            self.L.sphx_shm_abort(self.shm)

    def close(self):
        if self.shm:
            self.L.sphx_shm_close(self.shm)
            self.shm = None


class MultiSolver:
    def __init__(self, params, devices=None, halo=16, fixed_halo=False, rebalance_every=16, layout=_lib.LAYOUT_AUTO, cap_records=0,
                 overlap_exchange=False, _rank=None):
        self.L = _lib.lib()
        self.params = params
        o = SphxMultiOptions()
        self.L.sphx_multi_default_options(C.byref(o))
        o.halo_cells, o.fixed_halo, o.rebalance_every, o.layout, o.cap_records = halo, int(fixed_halo), rebalance_every, layout, cap_records
        o.overlap_exchange = int(overlap_exchange)
        self.options = o
        h = C.c_void_p()
        if _rank is None:
            devs = (C.c_int * len(devices))(*devices)
            rc = self.L.sphx_multi_create(C.byref(params), devs, len(devices), C.byref(o), C.byref(h))
        else:
            device, comm, job, rank, world = _rank
            self._comm = comm  # keeps the callbacks alive
            rc = self.L.sphx_multi_create_rank(C.byref(params), device, C.byref(comm.ops) if comm is not None else None,
                                               str(job).encode() if job is not None else None, rank, world, C.byref(o), C.byref(h))
        if rc:
            raise SphxError(rc, self.L.sphx_multi_last_error(None).decode())
        self.h = h

    @classmethod
    def rank(cls, params, device, rank, world, comm=None, job=None, **kw):
        """One tile of a multi-process run.  comm: TorchCommOps, or None for the library's own RCCL + shared-memory transport."""
        return cls(params, _rank=(device, comm, job, rank, world), **kw)

    def close(self):
        if getattr(self, "h", None):
            if not getattr(self, "_borrowed", False):  # (DFSPHMultiSolver.multi(): the solver object owns the tiles)
                self.L.sphx_multi_destroy(self.h)
            self.h = None

    __del__ = close

    def _chk(self, rc):
        if rc:
            msg = self.L.sphx_multi_last_error(self.h).decode()
            comm = getattr(self, "_comm", None)
            if comm is not None and comm.error is not None:
                msg += f" (communicator: {comm.error!r})"
            raise SphxError(rc, msg)

    def set_strips(self, axis, cuts):
        c = np.ascontiguousarray(cuts, np.uint32)
        self._chk(self.L.sphx_multi_set_layout(self.h, axis, _p(c), len(c)))

    def set_grid(self, xcuts, ycuts):
        x = np.ascontiguousarray(xcuts, np.uint32)
        yc = np.ascontiguousarray(ycuts, np.uint32)
        self._chk(self.L.sphx_multi_set_grid_layout(self.h, len(x) - 1, yc.shape[1] - 1, _p(x), _p(yc)))

    def set_boundary(self, xy):
        xy = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
        self._chk(self.L.sphx_multi_set_boundary(self.h, _p(xy), len(xy)))

    def upload(self, pos, vel=None, ids=None):
        pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 2)
        vel = np.ascontiguousarray(vel, np.float32).reshape(-1, 2) if vel is not None else None
        ids = np.ascontiguousarray(ids, np.uint32) if ids is not None else None
        self._chk(self.L.sphx_multi_upload(self.h, _p(pos), _p(vel), _p(ids), len(pos)))

    def clear_cached(self):
        self._chk(self.L.sphx_multi_clear_cached(self.h))

    def step_begin(self, dt_prev):
        v = C.c_float()
        self._chk(self.L.sphx_multi_step_begin(self.h, dt_prev, C.byref(v)))
        return v.value

    def step_finish(self, dt):
        st = SphxStepStats()
        self._chk(self.L.sphx_multi_step_finish(self.h, dt, C.byref(st)))
        return st.as_dict()

    def step(self, timer, diameter=np.float32(0.01)):
        """Solver::simulation_step with the host mirror of the caller's TimeManager in the middle (dfsph.rs:478-480)."""
        st = SphxStepStats()
        self._chk(self.L.sphx_multi_simulation_step(self.h, timer.h, diameter, C.byref(st)))
        d = st.as_dict()
        d["dt_ns"] = timer.simulation_step_ns()
        return d

    def steps(self, timer, k, diameter=np.float32(0.01)):
        """k consecutive step() calls inside the library (the frame loop of main.rs:348-350); returns the k stats dicts."""
        st = (SphxStepStats * k)()
        done = C.c_uint32()
        self._chk(self.L.sphx_multi_simulation_steps(self.h, timer.h, diameter, k, st, C.byref(done)))
        return [x.as_dict() for x in st]

    def synchronize(self):
        self._chk(self.L.sphx_multi_synchronize(self.h))

    def download(self):
        n = C.c_uint64(self.L.sphx_multi_num_owned(self.h) + 1024)
        for _ in range(2):
            cap = n.value
            pos, vel = np.zeros((cap, 2), np.float32), np.zeros((cap, 2), np.float32)
            den, ids = np.zeros(cap, np.float32), np.zeros(cap, np.uint32)
            rc = self.L.sphx_multi_download(self.h, _p(pos), _p(vel), _p(den), _p(ids), C.byref(n))
            if rc != _lib.ERR_CAPACITY:
                break
        self._chk(rc)
        k = n.value
        return dict(pos=pos[:k], vel=vel[:k], density=den[:k], ids=ids[:k])

    def info(self):
        i = SphxMultiInfo()
        self._chk(self.L.sphx_multi_info(self.h, C.byref(i)))
        d = {k: getattr(i, k) for k, _ in i._fields_ if k not in ("reserved", "transport")}
        d["transport"] = i.transport.decode()
        return d

    # ---- emitting and draining fluid (the contract is in include/sphx.h, "emitting and draining fluid in a tiled run") ----
    def append(self, pos, vel=None):
        """sphx_multi_append: add particles to the tiled run on the device (vel None = zero): each record goes to the tile that owns its
        cell, one halo exchange + re-grid follows.  Ids, warm-start sums and iteration counts of the run survive. -> the id of the first
        new particle.  Collective in rank mode (every rank passes the same records)."""
        from . import _append_arrays

        pos, vel = _append_arrays(pos, vel)
        first = C.c_uint32()
        self._chk(self.L.sphx_multi_append(self.h, _p(pos), _p(vel), len(pos), C.byref(first)))
        return first.value

    def remove(self, rects, outside=False):
        """sphx_multi_remove: drop the particles inside any of the rectangles (SphxContext.remove's predicate; outside=True: a keep-box)
        from the tiled run -> the number removed over all tiles.  Nothing removed: the run is untouched; else one halo exchange + re-grid.
        Collective in rank mode (every rank gets the same count)."""
        from . import _rect_array

        arr, k = _rect_array(rects)
        removed = C.c_uint64()
        self._chk(self.L.sphx_multi_remove(self.h, arr, k, _lib.REMOVE_OUTSIDE if outside else 0, C.byref(removed)))
        return removed.value

    # ---- fluid statistics of the tiled run (the contract is in include/sphx.h, "fluid statistics of a tiled run") ----
    def stats(self, rects=(), per_tile=False):
        """sphx_multi_fluid_stats: the records of SphxContext.stats() over the particles the tiles own, folded over the tiles in ascending
        rank — a structured array [1 + len(rects)] of STATS_DTYPE; per_tile=True: (that, the tiles' own records [world, 1 + len(rects)]).
        No download: every tile streams its arrays once on its own device.  Collective in rank mode (every rank gets the same bytes)."""
        from . import STATS_DTYPE, _rect_array

        arr, k = _rect_array(rects)
        rec = np.zeros(1 + k, STATS_DTYPE)
        tiles = np.zeros((self.info()["world"], 1 + k), STATS_DTYPE) if per_tile else None
        self._chk(self.L.sphx_multi_fluid_stats(self.h, arr, k, 0, _p(rec), _p(tiles)))
        return (rec, tiles) if per_tile else rec

    def stats_record(self, rects, max_frames, every=1):
        """sphx_multi_stats_record: from now on every `every`-th finished multi step makes each tile store one frame of its records on its
        device, up to max_frames frames (later ones are counted in stats_status()["dropped"]); max_frames=0 stops and frees.  Nothing
        is synchronised and nothing comes back until stats_frames()."""
        from . import _rect_array

        arr, k = _rect_array(rects)
        self._chk(self.L.sphx_multi_stats_record(self.h, arr, k, max_frames, every))

    def stats_status(self):
        """sphx_multi_stats_get_status -> dict(n_rects, recording, max_frames, every, frames, dropped)."""
        st = _lib.SphxStatsStatus()
        self._chk(self.L.sphx_multi_stats_get_status(self.h, C.byref(st)))
        return {k: getattr(st, k) for k, _ in st._fields_ if k != "reserved"}

    def stats_frames(self, first=0, count=None):
        """sphx_multi_stats_read -> (records [count, 1 + n_rects] of STATS_DTYPE, each frame folded over the tiles; info [count] of
        STATS_FRAME_DTYPE: step, dt, n) for the recorded frames [first, first + count) (count=None: all from `first`).  Waits for the
        tiles' streams; collective in rank mode."""
        from . import STATS_DTYPE, STATS_FRAME_DTYPE

        st = self.stats_status()
        if count is None:
            count = max(st["frames"] - first, 0)
        rec = np.zeros((count, 1 + st["n_rects"]), STATS_DTYPE)
        info = np.zeros(count, STATS_FRAME_DTYPE)
        self._chk(self.L.sphx_multi_stats_read(self.h, first, count, _p(rec) if count else None, _p(info) if count else None))
        return rec, info

    # ---- following particles by id (the contract is in include/sphx.h, "following particles by id in a tiled run") ----
    def track(self, ids):
        """sphx_multi_track_set: the ids to follow (any order, duplicates allowed, at most _lib.TRACK_MAX_IDS; an empty sequence clears
        the set).  Discards a recording.  The set belongs to the multi: it survives migration, re-partitioning, edits, uploads and
        state loads."""
        ids = np.ascontiguousarray(ids, np.uint32).reshape(-1)
        self._chk(self.L.sphx_multi_track_set(self.h, _p(ids) if len(ids) else None, len(ids)))

    def track_status(self):
        """sphx_multi_track_get_status -> dict(m, recording, max_frames, every, frames, dropped)."""
        st = _lib.SphxTrackStatus()
        self._chk(self.L.sphx_multi_track_get_status(self.h, C.byref(st)))
        return {k: getattr(st, k) for k, _ in st._fields_ if k != "reserved"}

    def track_fetch(self, fields=None):
        """sphx_multi_track_fetch: where the tracked particles are now, in the order of track(ids), without a download of the tiles:
        {"tile": uint32 [m] (the tile that owns the id), "slot": uint32 [m] (its index in tile_context(tile).download()), "pos":
        float32 [m, 2], "vel": float32 [m, 2], "density": float32 [m]} (or the requested `fields`).  An id no tile owns has tile and
        slot _lib.TRACK_ABSENT and NaN records (the word 0x7FC00000).  Rank mode: this rank's part, without communication — fold the
        ranks' parts with yasph2d_amd.track_merge."""
        from . import _multi_track_outputs, _multi_track_struct

        outs = _multi_track_outputs(fields, self.track_status()["m"])
        self._chk(self.L.sphx_multi_track_fetch(self.h, 0, C.byref(_multi_track_struct(outs))))
        return outs

    def track_record(self, max_frames, every=1):
        """sphx_multi_track_record: from now on every `every`-th finished multi step makes each tile store one frame of the tracked ids
        it owns on its device, up to max_frames frames (later ones are counted in track_status()["dropped"]); max_frames=0 stops and
        frees.  Works inside steps(timer, k) too; nothing is synchronised and nothing comes back until track_frames()."""
        self._chk(self.L.sphx_multi_track_record(self.h, max_frames, every))

    def track_frames(self, first=0, count=None, tiles=False):
        """sphx_multi_track_read -> float32 [count, m, 4] = x, y, vx, vy of the recorded frames [first, first + count) (count=None: all
        from `first`), folded over the local tiles; tiles=True: (that, uint32 [count, m]: the tile that owned each id then, or
        _lib.TRACK_ABSENT).  Rank mode: this rank's part — fold with yasph2d_amd.track_merge_frames."""
        st = self.track_status()
        if count is None:
            count = max(st["frames"] - first, 0)
        out = np.zeros((count, st["m"], 4), np.float32)
        til = np.zeros((count, st["m"]), np.uint32) if tiles else None
        self._chk(self.L.sphx_multi_track_read(self.h, first, count, 0, (out.ctypes.data or 1) if count else None,
                                               (til.ctypes.data or 1) if tiles and count else None))
        return (out, til) if tiles else out

    def download_by_id(self, first=0, count=None, fields=None):
        """sphx_multi_download_by_id: the particles with the ids first .. first + count - 1 in id order -> the dict of track_fetch()
        plus "present", the number of ids found.  count=None: up to the largest id the local tiles own (one sphx_multi_download of the
        ids; pass count where that matters).  After an unedited upload(pos) it is the particles in upload order, whatever the steps
        and migrations since.  Every tile returns only the records it owns."""
        from . import _multi_track_outputs, _multi_track_struct

        if count is None:
            n = C.c_uint64(self.L.sphx_multi_num_owned(self.h))
            ids = np.zeros(n.value, np.uint32)
            self._chk(self.L.sphx_multi_download(self.h, None, None, None, _p(ids) if n.value else None, C.byref(n)))
            count = max(int(ids[:n.value].max()) + 1 - first, 0) if n.value else 0
        outs = _multi_track_outputs(fields, count)
        present = C.c_uint32()
        self._chk(self.L.sphx_multi_download_by_id(self.h, first, count, 0, C.byref(_multi_track_struct(outs)), C.byref(present)))
        outs["present"] = present.value
        return outs

    # ---- sampling the fields of the tiled run (the contract is in include/sphx.h, "sampling the fields of a tiled run") ----
    def _sample_outputs(self, fields, shape, tiles):
        from . import _numpy_outputs, _sample_fields

        outs = _numpy_outputs(_sample_fields(fields), shape)
        if tiles or self.info()["local_tiles"] < self.info()["world"]:  # (a rank of a multi-process run: tile says what it answered)
            outs["tile"] = np.full(shape, -1, np.int32)
        o = _lib.SphxMultiSampleOut()
        for f, a in outs.items():
            setattr(o, f, a.ctypes.data or 1)  # (an empty array: a non-NULL dummy still names the field; nothing is written)
        return outs, o

    def sample(self, points, kernel=_lib.KERNEL_WENDLAND_C2, fields=SAMPLE_FIELDS, tiles=False):
        """sphx_multi_sample_points: the fields at m query points (float32 [m, 2], numpy), each answered by the tile that owns the
        point's cell, over that tile's own arrays — no download.  Returns {field: array} with the shapes and dtypes of
        SphxContext.sample (host path); tiles=True adds "tile": int32 [m], the tile that answered.  If the ghost band is spent, the
        halo exchange the next step owes happens now (collective in rank mode: every rank calls with the same points).  Rank mode:
        this rank's part — zeros and tile -1 for the points other ranks answer ("tile" is always returned); fold the ranks' parts
        with yasph2d_amd.sample_merge."""
        pts = np.ascontiguousarray(points, np.float32)
        if pts.ndim != 2 or pts.shape[1] != 2:
            raise ValueError("points must be a float32 [m, 2] array, not shape %s" % (pts.shape,))
        outs, o = self._sample_outputs(fields, (len(pts),), tiles)
        self._chk(self.L.sphx_multi_sample_points(self.h, _p(pts), len(pts), kernel, 0, C.byref(o)))
        return outs

    def sample_grid(self, origin, spacing, shape, kernel=_lib.KERNEL_WENDLAND_C2, fields=SAMPLE_FIELDS, tiles=False):
        """sphx_multi_sample_grid: the fields on the lattice origin + (ix * dx, iy * dy) (fp32, unfused), shape = (ny, nx), row 0 at
        origin[1]; arguments and result as SphxContext.sample_grid, bit-identical to sample() at the same fp32 points.  Every tile
        walks only the index rectangle of the lattice it owns.  tiles, the ghost band and rank mode: as sample()."""
        dx, dy = (spacing, spacing) if np.ndim(spacing) == 0 else spacing
        ny, nx = (int(v) for v in shape)
        if nx < 0 or ny < 0:
            raise ValueError("shape must be (ny, nx) with non-negative sizes")
        outs, o = self._sample_outputs(fields, (ny, nx), tiles)
        self._chk(self.L.sphx_multi_sample_grid(self.h, origin[0], origin[1], dx, dy, nx, ny, kernel, 0, C.byref(o)))
        return outs

    # ---- gauges and probes of the tiled run (the contract is in include/sphx.h, "gauges and probes of a tiled run") ----
    def gauges(self, gauges, iso=0.5, field="fraction", kernel=_lib.KERNEL_WENDLAND_C2, values=False, tiles=False):
        """sphx_multi_gauge_levels: SphxContext.gauges for the tiled run — every sample is answered by the tile that owns its cell, each
        tile reduces the samples it owns on its device, and the 32-byte parts are folded on the host: no sample value crosses unless
        values=True asks for them.  Returns the GAUGE_REC_DTYPE array [g]; with values=True and / or tiles=True a tuple that adds the
        float32 values [sum n] and / or the tiles' parts (GAUGE_PART_DTYPE [local tiles, g]), in that order.  If the ghost band is spent,
        the halo exchange the next step owes happens now (collective in rank mode).  Rank mode: the records are None and the parts are
        always returned; fold the ranks' parts with yasph2d_amd.gauge_merge."""
        from . import GAUGE_PART_DTYPE, GAUGE_REC_DTYPE, _gauge_array

        if field not in _lib.GAUGE_FIELDS:
            raise ValueError("field must be one of %s, not %r" % (sorted(_lib.GAUGE_FIELDS), field))
        g = _gauge_array(gauges)
        total = int(g["n"].astype(np.int64).sum())
        rank_mode = self._in_rank_mode()
        rec = np.zeros(len(g), GAUGE_REC_DTYPE)
        val = np.zeros(total, np.float32) if values else None
        parts = np.zeros((self.info()["local_tiles"], len(g)), GAUGE_PART_DTYPE) if tiles or rank_mode else None
        self._chk(self.L.sphx_multi_gauge_levels(self.h, _p(g) if len(g) else None, len(g), kernel, _lib.GAUGE_FIELDS[field], iso, 0,
                                                 rec.ctypes.data or 1, (val.ctypes.data or 1) if values else None,
                                                 (parts.ctypes.data or 1) if parts is not None else None))
        res = (None if rank_mode else rec,) + ((val,) if values else ()) + ((parts,) if parts is not None else ())
        return res[0] if len(res) == 1 else res

    def probe_record(self, points=None, gauges=None, max_frames=0, every=1, iso=0.5, field="fraction", kernel=_lib.KERNEL_WENDLAND_C2):
        """sphx_multi_probe_record: from now on every `every`-th finished multi step stores one frame on every tile's device —
        sample(points)' four fields at the fixed points and the parts of gauges(gauges, iso, field, kernel) — up to max_frames frames
        (later ones are counted in probe_status()["dropped"]); max_frames=0 stops and frees.  Works inside steps(timer, k) and may be
        called before the first upload; nothing is synchronised beyond the halo exchange a frame may pull forward."""
        from . import _gauge_array

        if field not in _lib.GAUGE_FIELDS:
            raise ValueError("field must be one of %s, not %r" % (sorted(_lib.GAUGE_FIELDS), field))
        g = _gauge_array(gauges)
        pts = np.zeros((0, 2), np.float32) if points is None else np.ascontiguousarray(points, np.float32)
        if pts.ndim != 2 or pts.shape[1] != 2:
            raise ValueError("points must be a float32 [m, 2] array, not shape %s" % (pts.shape,))
        self._chk(self.L.sphx_multi_probe_record(self.h, _p(pts) if len(pts) else None, len(pts), _p(g) if len(g) else None, len(g), kernel,
                                                 _lib.GAUGE_FIELDS[field], iso, max_frames, every))

    def probe_status(self):
        """sphx_multi_probe_get_status -> dict(m_points, n_gauges, recording, max_frames, every, frames, dropped)."""
        st = _lib.SphxProbeStatus()
        self._chk(self.L.sphx_multi_probe_get_status(self.h, C.byref(st)))
        return {k: getattr(st, k) for k, _ in st._fields_ if k != "reserved"}

    def probe_frames(self, first=0, count=None, tiles=False):
        """sphx_multi_probe_read -> dict(points [count, m_points] of PROBE_REC_DTYPE, gauges [count, n_gauges] of GAUGE_REC_DTYPE, info
        [count] of STATS_FRAME_DTYPE) for the recorded frames [first, first + count) (count=None: all from `first`), folded over the
        tiles; tiles=True adds "point_tile": int32 [count, m_points], the tile that answered each point (-1: none).  Waits for the
        tiles' streams.  Rank mode: "points" and "point_tile" are this rank's part, "gauges" is None and "parts" holds the rank's
        GAUGE_PART_DTYPE [count, n_gauges] (fold each frame with yasph2d_amd.gauge_merge)."""
        from . import GAUGE_PART_DTYPE, GAUGE_REC_DTYPE, PROBE_REC_DTYPE, STATS_FRAME_DTYPE

        st = self.probe_status()
        if count is None:
            count = max(st["frames"] - first, 0)
        rank_mode = self._in_rank_mode()
        pts = np.zeros((count, st["m_points"]), PROBE_REC_DTYPE)
        til = np.full((count, st["m_points"]), -1, np.int32) if tiles or rank_mode else None
        gau = None if rank_mode else np.zeros((count, st["n_gauges"]), GAUGE_REC_DTYPE)
        info = np.zeros(count, STATS_FRAME_DTYPE)
        self._chk(self.L.sphx_multi_probe_read(self.h, first, count, _p(pts) if pts.size else None, _p(til) if til is not None and til.size else None,
                                               _p(gau) if gau is not None and gau.size else None, _p(info) if count else None))
        res = dict(points=pts, gauges=gau, info=info)
        if til is not None:
            res["point_tile"] = til
        if rank_mode:
            parts = np.zeros((count, st["n_gauges"]), GAUGE_PART_DTYPE)
            if parts.size:
                ctx = self.tile_context(0)
                ctx._chk(self.L.sphx_tile_probe_read(ctx.h, first, count, None, _p(parts), None))
            res["parts"] = parts
        return res

    # ---- the free surface of the tiled run (the contract is in include/sphx.h, "free surface of a tiled run") ----
    def contour(self, origin, spacing, shape, iso=0.5, field="fraction", kind=_lib.KERNEL_WENDLAND_C2, cap=None, tiles=False):
        """sphx_multi_surface_contour: the contour `field == iso` of the lattice sample_grid(origin, spacing, shape) returns, cut by the
        tiles on their devices — no download, and the lattice does not cross to the host.  Arguments and result as
        SphxContext.contour (host path): dict(segments [n, 2, 2], cell [n], count), in ascending cell order; tiles=True adds "tile":
        int32 [n], the tile that cut the segment's cell.  cap=None makes two calls, the count first and then the exact capacity, so
        n = count; cap = 0 returns the count alone.  If the ghost band is spent, the halo exchange the next step owes happens now
        (collective in rank mode).  Rank mode: this rank's part ("tile" is always returned; n = min(count of this rank, cap)); fold the
        ranks' parts with yasph2d_amd.contour_merge."""
        if field not in _lib.CONTOUR_FIELDS:
            raise ValueError("field must be one of %s, not %r" % (sorted(_lib.CONTOUR_FIELDS), field))
        dx, dy = (spacing, spacing) if np.ndim(spacing) == 0 else spacing
        ny, nx = (int(v) for v in shape)
        if nx < 0 or ny < 0:
            raise ValueError("shape must be (ny, nx) with non-negative sizes")
        want_tile = tiles or self.info()["local_tiles"] < self.info()["world"]
        cnt = np.zeros(1, np.uint32)

        def call(cap_):
            seg, cel, til = np.zeros((cap_, 2, 2), np.float32), np.zeros(cap_, np.uint32), np.full(cap_, -1, np.int32)
            o = _lib.SphxMultiContourOut()
            o.count = cnt.ctypes.data
            if cap_:
                o.segments, o.cell = seg.ctypes.data, cel.ctypes.data
                o.tile = til.ctypes.data if want_tile else None
            self._chk(self.L.sphx_multi_surface_contour(self.h, origin[0], origin[1], dx, dy, nx, ny, kind, _lib.CONTOUR_FIELDS[field], iso, cap_, 0, C.byref(o)))
            return seg, cel, til

        if cap is None:
            call(0)
            cap = int(cnt[0])
        cap = int(cap)
        seg, cel, til = call(cap)
        count = int(cnt[0])
        n = min(count, cap)
        res = dict(segments=seg[:n], cell=cel[:n], count=count)
        if want_tile:
            res["tile"] = til[:n]
        return res

    # ---- neighbour queries of the tiled run (the contract is in include/sphx.h, "neighbour queries of a tiled run") ----
    def _in_rank_mode(self):
        i = self.info()
        return i["local_tiles"] < i["world"]

    def query(self, points, radius=None, boundary=False, lists=True, nearest=True, cap=None, tiles=False):
        """sphx_multi_query_radius: the particles within `radius` of m query points (float32 [m, 2], numpy), each point answered by the
        tile that owns its cell over that tile's own arrays, ghosts included — no download.  radius: None = the smoothing length h.
        boundary=True answers over the boundary particles instead of the fluid.
        Returns dict(offsets uint64 [m + 1] (CSR), count; with lists: id uint32 [n] (the particle id download() reports; boundary: the
        index in the array given to set_boundary), dist_sq float32 [n], slot uint32 [n] (the index in the answering tile's own
        download); with nearest: nearest_id, nearest_slot uint32 [m] (_lib.QUERY_NONE where nothing is accepted), nearest_dist_sq
        float32 [m] (+inf there); with tiles=True (always in rank mode): tile int32 [m], the tile that answered).  cap: the most entries
        to return (n = min(count, cap)); None makes two calls, the count first, so n = count.
        Nothing is exchanged and the run is untouched; the call is not collective.  Rank mode: this rank's part — empty ranges, tile -1
        and no nearest for the points other ranks answer; fold the ranks' parts with yasph2d_amd.query_merge."""
        if radius is None and self.params is None:
            raise ValueError("radius=None needs the params the multi was created with (a borrowed view has none): pass the radius")
        r = float(np.float32(self.params.smoothing_length if radius is None else radius))
        pts = np.ascontiguousarray(points, np.float32)
        if pts.ndim != 2 or pts.shape[1] != 2:
            raise ValueError("points must be a float32 [m, 2] array, not shape %s" % (pts.shape,))
        m = len(pts)
        flags = _lib.QUERY_BOUNDARY if boundary else 0
        want_tile = tiles or self._in_rank_mode()
        cnt, off = np.zeros(1, np.uint64), np.zeros(m + 1, np.uint64)
        o = _lib.SphxMultiQueryOut()
        o.offsets, o.count = off.ctypes.data, cnt.ctypes.data
        res = dict(offsets=off)
        if nearest:
            res.update(nearest_id=np.full(m, _lib.QUERY_NONE, np.uint32), nearest_slot=np.full(m, _lib.QUERY_NONE, np.uint32),
                       nearest_dist_sq=np.full(m, np.inf, np.float32))
            for f in ("nearest_id", "nearest_slot", "nearest_dist_sq"):
                setattr(o, f, res[f].ctypes.data or 1)
        if want_tile:
            res["tile"] = np.full(m, -1, np.int32)
            o.tile = res["tile"].ctypes.data or 1
        cap_ = int(cap) if cap is not None else 0
        if cap is None or not lists:
            self._chk(self.L.sphx_multi_query_radius(self.h, _p(pts), m, r, 0, flags, C.byref(o)))  # count only: one walk
            cap_ = int(cnt[0]) if cap is None else cap_
        if lists:
            ids, d2, slot = np.zeros(cap_, np.uint32), np.zeros(cap_, np.float32), np.zeros(cap_, np.uint32)
            if cap is not None or cap_:
                o.id, o.dist_sq, o.slot = (ids.ctypes.data, d2.ctypes.data, slot.ctypes.data) if cap_ else (None, None, None)
                self._chk(self.L.sphx_multi_query_radius(self.h, _p(pts), m, r, cap_, flags, C.byref(o)))
            n = min(int(cnt[0]), cap_)
            res.update(id=ids[:n], dist_sq=d2[:n], slot=slot[:n])
        res["count"] = int(cnt[0])
        return res

    def select(self, rects, outside=False, cap=None, by_id=False):
        """sphx_multi_select: the particles sphx_multi_remove(rects, outside) would remove — and nothing is removed.  Every tile answers
        for the particles it owns; the result is in the order of download().  Returns dict(id uint32 [n], tile int32 [n] (the owning
        tile), slot uint32 [n] (the index in tile_context(tile).download()), count).  cap: the most to return (n = min(count, cap));
        None makes two calls, the count first.  by_id=True sorts the rows by id on the host.  Rank mode: this rank's part; the whole
        answer is the ranks' parts concatenated in rank order."""
        from . import _rect_array

        arr, k = _rect_array(rects)
        flags = _lib.SELECT_OUTSIDE if outside else 0
        cnt = np.zeros(1, np.uint64)
        o = _lib.SphxMultiSelectOut()
        o.count = cnt.ctypes.data
        if cap is None:
            self._chk(self.L.sphx_multi_select(self.h, arr, k, flags, 0, C.byref(o)))
            cap_ = int(cnt[0])
        else:
            cap_ = int(cap)
        ids, til, slot = np.zeros(cap_, np.uint32), np.full(cap_, -1, np.int32), np.zeros(cap_, np.uint32)
        if cap_:
            o.id, o.tile, o.slot = ids.ctypes.data, til.ctypes.data, slot.ctypes.data
        if cap is not None or cap_:
            self._chk(self.L.sphx_multi_select(self.h, arr, k, flags, cap_, C.byref(o)))
        n = min(int(cnt[0]), cap_)
        res = dict(id=ids[:n], tile=til[:n], slot=slot[:n])
        if by_id:
            order = np.argsort(res["id"], kind="stable")
            res = {f: a[order] for f, a in res.items()}
        res["count"] = int(cnt[0])
        return res

    # ---- per-particle flow fields of the tiled run (the contract is in include/sphx.h, "per-particle flow fields of a tiled run") ----
    def fields(self, fields=None, by_id=False):
        """sphx_multi_particle_fields: velocity gradient, divergence, vorticity and colour-field gradient (SphxContext.fields) at every
        particle the local tiles own, each computed by its tile over the tile's own arrays — no download, no second context.  Returns
        {name: numpy float32 array} for the requested `fields` (default: yasph2d_amd.FIELD_NAMES; shapes as SphxContext.fields) plus
        "ids" (uint32 [n]: the particle id of row k) and "tile" (int32 [n]: the tile that owns it).  Row k belongs to row k of a
        download() made AFTER the call and before the next step; by_id=True sorts the rows by id on the host instead.  If the ghost
        band is spent, the halo exchange the next step owes happens now (collective in rank mode).  Rank mode: this rank's part; the
        whole answer is the ranks' parts concatenated in rank order."""
        from . import _FIELD_SHAPE, FIELD_NAMES, _field_names

        names = _field_names(FIELD_NAMES if fields is None else fields)
        n = C.c_uint64(self.L.sphx_multi_num_owned(self.h) + 1024)
        for _ in range(2):  # (the host's owned count lags a migration: the call reports the count it needs)
            cap = n.value
            outs = {f: np.zeros((cap,) + _FIELD_SHAPE[f], np.float32) for f in names}
            outs["ids"], outs["tile"] = np.zeros(cap, np.uint32), np.zeros(cap, np.int32)
            o = _lib.SphxMultiFieldsOut()
            for f, a in outs.items():
                setattr(o, f, a.ctypes.data or 1)
            rc = self.L.sphx_multi_particle_fields(self.h, 0, C.byref(o), C.byref(n))
            if rc != _lib.ERR_CAPACITY:
                break
        self._chk(rc)
        k = n.value
        outs = {f: a[:k] for f, a in outs.items()}
        if by_id:
            order = np.argsort(outs["ids"], kind="stable")
            outs = {f: a[order] for f, a in outs.items()}
        return outs

    def tile_rects(self):
        """sphx_multi_tile_rects -> uint32 [world, 4]: the owned cell rectangle (x0, x1, y0, y1), half-open, of every tile in rank order."""
        n = C.c_uint32(self.info()["world"])
        arr = (_lib.SphxTileRect * max(n.value, 1))()
        rc = self.L.sphx_multi_tile_rects(self.h, arr, C.byref(n))
        if rc:
            raise SphxError(rc, "sphx_multi_tile_rects: no layout before the first upload" if rc == _lib.ERR_NOT_READY else "sphx_multi_tile_rects")
        return np.array([(r.x0, r.x1, r.y0, r.y1) for r in arr[:n.value]], np.uint32).reshape(-1, 4)

    def ghost_rings(self):
        """sphx_multi_ghost_rings -> dict(valid, kvalid, avalid): the ring budget of local tile 0 (rings of ghosts, counted from the
        owned region, in which velocities / warm-start sums / densities are still exact; inf on a one-tile run)."""
        out = (C.c_double * 3)()
        self._chk(self.L.sphx_multi_ghost_rings(self.h, out))
        return dict(valid=out[0], kvalid=out[1], avalid=out[2])

    # ---- picture of the tiled run (the contract is in include/sphx.h, "picture of a tiled run") ----
    @staticmethod
    def _view(view, view_fields):
        from . import SCENE_RECT, _copy_view, _set_view_fields, render_fit

        if view is None:
            width, height = view_fields.pop("width", 1920), view_fields.pop("height", 1080)
            view = render_fit(width, height, view_fields.pop("world_rect", SCENE_RECT))
        else:
            view = _copy_view(view)
        return _set_view_fields(view, view_fields)

    def render(self, view=None, *, owner=False, rgba=True, **view_fields):
        """sphx_multi_render: the whole run drawn as SphxContext.render draws a single context (host path), without a download: every
        tile draws the particles it owns on its own device, the pictures are merged on the host.  Returns the uint8 (H, W, 4) image;
        with owner=True the pair (image, uint32 (H, W) owners: a particle ID, _lib.RENDER_BOUNDARY or _lib.RENDER_NONE); with
        rgba=False the owners alone.  In-process only: a rank of a multi-process run takes render_layer() and render_merge()."""
        view = self._view(view, view_fields)
        if not rgba and not owner:
            raise ValueError("nothing to render: rgba and owner are both off")
        h, w = view.height, view.width
        img = np.zeros((h, w, 4), np.uint8) if rgba else None
        own = np.zeros((h, w), np.uint32) if owner else None
        o = _lib.SphxRenderOut()
        o.rgba = (img.ctypes.data or 1) if rgba else None
        o.owner = (own.ctypes.data or 1) if owner else None
        self._chk(self.L.sphx_multi_render(self.h, C.byref(view), 0, C.byref(o)))
        return own if not rgba else ((img, own) if owner else img)

    def render_layer(self, view=None, **view_fields):
        """sphx_multi_render_layer -> dict(key uint32 (H, W), owner uint32 (H, W), rgba uint8 (H, W, 4)): the merged layer of the local
        tiles (in-process: all of them; rank mode: this rank's one).  No communication; layers of the ranks of one run are combined
        with yasph2d_amd.render_merge."""
        view = self._view(view, view_fields)
        h, w = view.height, view.width
        out = dict(key=np.zeros((h, w), np.uint32), owner=np.zeros((h, w), np.uint32), rgba=np.zeros((h, w, 4), np.uint8))
        o = _lib.SphxRenderLayer(*[(out[k].ctypes.data or 1) for k in ("key", "owner", "rgba")])
        self._chk(self.L.sphx_multi_render_layer(self.h, C.byref(view), 0, C.byref(o)))
        return out

    # ---- checkpoint of the tiled run (the contract is in include/sphx.h, "checkpoint of a tiled run") ----
    def save_state(self):
        """sphx_multi_state_save -> bytes: this process's part of the checkpoint (in-process: the whole run, part 0 of 1; rank mode: part
        rank of world).  Taken on the device from the particles the tiles own; two saves of one state are byte-identical."""
        n = C.c_uint64()
        self._chk(self.L.sphx_multi_state_size(self.h, C.byref(n)))
        buf = np.zeros(n.value, np.uint8)
        self._chk(self.L.sphx_multi_state_save(self.h, _p(buf), n.value, 0, C.byref(n)))
        return buf[:n.value].tobytes()

    def load_state(self, parts):
        """sphx_multi_state_load: `parts` is the bytes of one part or a list of all parts of a checkpoint (any order); every rank passes
        all of them.  The checkpoint may come from another tiling.  Replaces the particles, the boundary and the warm-start state."""
        if isinstance(parts, (bytes, bytearray, memoryview, np.ndarray)):
            parts = [parts]
        arrs = [np.frombuffer(bytes(b), np.uint8) if not isinstance(b, np.ndarray) else np.ascontiguousarray(b, np.uint8) for b in parts]
        k = len(arrs)
        ptrs = (C.c_void_p * max(k, 1))(*[a.ctypes.data for a in arrs])
        sizes = (C.c_uint64 * max(k, 1))(*[a.size for a in arrs])
        self._chk(self.L.sphx_multi_state_load(self.h, ptrs, sizes, k, 0))

    def state_digest(self):
        """sphx_multi_state_digest -> {section: digest} of the whole run (_lib.MULTI_STATE_SECTIONS): id-keyed for the particle sections,
        positional for the boundary.  64 bytes come back; collective in rank mode (every rank gets the same)."""
        out = (C.c_uint64 * len(_lib.MULTI_STATE_SECTIONS))()
        self._chk(self.L.sphx_multi_state_digest(self.h, out))
        return dict(zip(_lib.MULTI_STATE_SECTIONS, (int(v) for v in out)))

    def save_state_file(self, path):
        """sphx_multi_state_save_file (rank mode: the part goes to path + ".rRRRofWWW")."""
        self._chk(self.L.sphx_multi_state_save_file(self.h, str(path).encode()))

    def load_state_file(self, path):
        """sphx_multi_state_load_file: the one file, or the complete set of part files path.r000ofWWW ..."""
        self._chk(self.L.sphx_multi_state_load_file(self.h, str(path).encode()))

    def set_tiling_invariant(self, on=True):
        """sphx_set_tiling_invariant on every local tile: cell mates ordered by persistent id (the tiles' warm-start values always travel).
        A single context and the oracle in the same mode then compute the same run, bit for bit (a comparison mode)."""
        for k in range(self.info()["local_tiles"]):
            self.tile_context(k).set_tiling_invariant(on)

    def viscosity(self, k=0):
        """The viscosity model local tile k runs (SphxContext.viscosity): every tile context is created from the same params."""
        return self.tile_context(k).viscosity()

    def tile_context(self, k=0):
        """Borrowed SphxContext view of a local tile (inspection, profiling)."""
        from . import SphxContext

        ctx = SphxContext.__new__(SphxContext)
        ctx.L, ctx.params, ctx._owned = self.L, None, False
        ctx.h = C.c_void_p(self.L.sphx_multi_tile_ctx(self.h, k))
        return ctx
