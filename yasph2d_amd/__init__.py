"""yasph2d_amd — MI355X-native DFSPH step loop behind yasph2d's Solver / particle-array surface.

Python is only the test/bench driver here.  The product is libsphx.so (hand-written HIP for gfx950 + a C ABI,
include/sphx.h); the classes below are thin ctypes views of
  * the device solver context (`SphxContext`  — what a Rust `impl Solver` shim would bind), and
  * the C++ host-side mirror of the reference's caller types (`FluidParticleWorld`, `TimeManager`, `DFSPHSolver`),
named after the reference (src/sph/fluidparticleworld.rs, timemanager.rs, solver/dfsph.rs).
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import (FLAG_DENSITY_ITER_CAP, FLAG_DIVERGENCE_ITER_CAP, FLAG_DENSE_CELL, FLAG_NEIGHBOR_CAP, FLAG_STRAY_PARTICLES, FLAG_WARMUP, KERNEL_POLY6,  # noqa: F401
                   KERNEL_SPIKY, KERNEL_WENDLAND_C2, VISCOSITY_PHYSICAL, VISCOSITY_XSPH, SphxError, SphxKernelTime, SphxParams, SphxStepStats)

__all__ = ["SphxContext", "FluidParticleWorld", "TimeManager", "DFSPHSolver", "DFSPHMultiSolver", "default_params", "duration_from_secs_f32",
           "duration_as_secs_f32", "SphxError", "WCSPHSolver", "VISCOSITY_XSPH", "VISCOSITY_PHYSICAL", "SAMPLE_FIELDS", "gauge_elevation", "contour_chain", "contour_lines", "contour_merge",
           "sample_merge", "query_merge", "render_fit", "render_merge", "track_merge", "track_merge_frames", "write_png", "SCENE_RECT", "TRACK_FIELDS", "MULTI_TRACK_FIELDS", "FIELD_NAMES", "STATS_DTYPE", "STATS_FRAME_DTYPE",
           "GAUGE_DTYPE", "GAUGE_REC_DTYPE", "PROBE_REC_DTYPE", "gauge_reduce", "GAUGE_PART_DTYPE", "gauge_merge"]


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


LISTS_32BIT = 0xFFFFFFFF  # sphx_params.list_span_limit: never compress the neighbour lists


_VISCOSITY_MODELS = {"xsph": VISCOSITY_XSPH, "physical": VISCOSITY_PHYSICAL}


def default_params(smoothing_factor=2.0, particle_density=10000.0, fluid_density=100.0, device=0, fixed_iterations=(0, 0), viscosity="xsph",
                   fluid_viscosity=None):
    """sphx_default_params: the constants of the reference app (main.rs:85-89, dfsph.rs:49-55).

    viscosity: the solver's ViscosityModel, "xsph" (XSPHViscosityModel, main.rs:100) or "physical" (PhysicalViscosityModel,
    physical.rs); fluid_viscosity: its mu (None keeps the library default 1.0016e-3, physical.rs:14; main.rs:96 sets 0.01)."""
    if viscosity not in _VISCOSITY_MODELS:
        raise ValueError("viscosity must be one of %s, not %r" % (sorted(_VISCOSITY_MODELS), viscosity))
    p = SphxParams()
    rc = _lib.lib().sphx_default_params(smoothing_factor, particle_density, fluid_density, C.byref(p))
    if rc:
        raise SphxError(rc, "sphx_default_params")
    p.device = device
    p.fixed_density_iterations, p.fixed_divergence_iterations = fixed_iterations
    p.viscosity_model = _VISCOSITY_MODELS[viscosity]
    if fluid_viscosity is not None:
        p.fluid_viscosity = fluid_viscosity
    return p


def duration_from_secs_f32(secs):
    return _lib.lib().sphx_duration_from_secs_f32(secs)


def duration_as_secs_f32(ns):
    return _lib.lib().sphx_duration_as_secs_f32(ns)


SAMPLE_FIELDS = ("density", "fraction", "velocity", "count")


def _sample_fields(fields):
    fields = (fields,) if isinstance(fields, str) else tuple(fields)
    bad = [f for f in fields if f not in SAMPLE_FIELDS]
    if bad or not fields:
        raise ValueError("fields must be a non-empty subset of %s, not %r" % (SAMPLE_FIELDS, fields))
    return fields


def _is_torch(a):
    return type(a).__module__.split(".")[0] == "torch"


def _numpy_outputs(fields, shape):
    return {f: np.zeros(shape + ((2,) if f == "velocity" else ()), np.uint32 if f == "count" else np.float32) for f in fields}


def _torch_outputs(fields, shape, device):
    import torch

    return {f: torch.empty(shape + ((2,) if f == "velocity" else ()), dtype=torch.int32 if f == "count" else torch.float32, device=device)
            for f in fields}


def _out_struct(outs, ptr):
    o = _lib.SphxSampleOut()
    for f, a in outs.items():
        setattr(o, f, ptr(a) or 1)  # (an empty tensor has no storage: a non-NULL dummy still names the field; nothing is written)
    return o


def sample_merge(parts):
    """sphx_sample_merge: the parts the ranks of one run returned from MultiSolver.sample() or sample_grid() (dicts with "tile" and the
    same other fields, all of one shape) folded into the answer of the whole run: per point the part whose tile is >= 0 (the lowest
    tile if several are), zeros and tile -1 where none is.  -> the dict of the common fields, "tile" included.  Host code; no GPU."""
    parts = list(parts)
    if not parts:
        raise ValueError("sample_merge needs at least one part (the shape of the answer is the parts')")
    if any("tile" not in p for p in parts):
        raise ValueError("sample_merge: every part needs its \"tile\" array")
    shape = np.shape(parts[0]["tile"])
    m = int(np.prod(shape))
    fields = [f for f in SAMPLE_FIELDS if all(f in p for p in parts)]
    dtype = dict(density=np.float32, fraction=np.float32, velocity=np.float32, count=np.uint32, tile=np.int32)
    kept = []
    arr = (_lib.SphxMultiSampleOut * len(parts))()
    for k, p in enumerate(parts):
        a = {f: np.ascontiguousarray(p[f], dtype[f]) for f in fields + ["tile"]}
        if any(a[f].shape != shape + ((2,) if f == "velocity" else ()) for f in a):
            raise ValueError("sample_merge: the parts differ in shape")
        kept.append(a)
        for f, v in a.items():
            setattr(arr[k], f, v.ctypes.data or 1)
    outs = _numpy_outputs(fields, shape)
    outs["tile"] = np.full(shape, -1, np.int32)
    o = _lib.SphxMultiSampleOut()
    for f, v in outs.items():
        setattr(o, f, v.ctypes.data or 1)
    L = _lib.lib()
    rc = L.sphx_sample_merge(m, arr, len(parts), C.byref(o))
    if rc:
        raise SphxError(rc, L.sphx_multi_last_error(None).decode())
    return outs


TRACK_FIELDS = ("slot", "pos", "vel", "density")


def _track_outputs(fields, m):
    fields = (fields,) if isinstance(fields, str) else tuple(fields)
    bad = [f for f in fields if f not in TRACK_FIELDS]
    if bad or not fields:
        raise ValueError("fields must be a non-empty subset of %s, not %r" % (TRACK_FIELDS, fields))
    return {f: np.zeros((m, 2) if f in ("pos", "vel") else (m,), np.uint32 if f == "slot" else np.float32) for f in fields}


def _track_struct(outs):
    o = _lib.SphxTrackOut()
    for f, a in outs.items():
        setattr(o, f, a.ctypes.data or 1)  # (an empty array: a non-NULL dummy still names the field; nothing is written)
    return o


MULTI_TRACK_FIELDS = ("tile", "slot", "pos", "vel", "density")  # sphx_multi_track_out


def _multi_track_outputs(fields, m):
    fields = MULTI_TRACK_FIELDS if fields is None else ((fields,) if isinstance(fields, str) else tuple(fields))
    bad = [f for f in fields if f not in MULTI_TRACK_FIELDS]
    if bad or not fields:
        raise ValueError("fields must be a non-empty subset of %s, not %r" % (MULTI_TRACK_FIELDS, fields))
    return {f: np.zeros((m, 2) if f in ("pos", "vel") else (m,), np.uint32 if f in ("tile", "slot") else np.float32) for f in fields}


def _multi_track_struct(outs):
    o = _lib.SphxMultiTrackOut()
    for f in MULTI_TRACK_FIELDS:
        if f in outs:
            setattr(o, f, outs[f].ctypes.data or 1)  # (an empty array: a non-NULL dummy still names the field; nothing is written)
    return o


def track_merge(parts):
    """sphx_track_merge: the parts the ranks of one run returned from MultiSolver.track_fetch() or download_by_id() (dicts with "tile",
    "slot" and the same other fields, all of one length) folded into the answer of the whole run: per id the part that holds it (the
    greatest (tile, slot) if several do), else absent.  -> the dict of the common fields plus "present".  Host code; no GPU needed."""
    parts = list(parts)
    if not parts:
        raise ValueError("track_merge needs at least one part (the number of ids is the parts')")
    fields = [f for f in MULTI_TRACK_FIELDS if all(f in p for p in parts)]
    m = len(parts[0]["tile"]) if "tile" in parts[0] else 0
    kept = []
    arr = (_lib.SphxMultiTrackOut * len(parts))()
    for k, p in enumerate(parts):
        a = {f: np.ascontiguousarray(p[f], np.uint32 if f in ("tile", "slot") else np.float32) for f in fields}
        if any(a[f].size != m * (2 if f in ("pos", "vel") else 1) for f in fields):
            raise ValueError("track_merge: the parts differ in length")
        kept.append(a)
        for f in fields:
            setattr(arr[k], f, a[f].ctypes.data or 1)
    outs = _multi_track_outputs(fields or ("tile",), m)
    present = C.c_uint32()
    L = _lib.lib()
    rc = L.sphx_track_merge(m, arr, len(parts), C.byref(_multi_track_struct(outs)), C.byref(present))
    if rc:
        raise SphxError(rc, L.sphx_multi_last_error(None).decode())
    outs["present"] = present.value
    return outs


def track_merge_frames(parts):
    """sphx_track_merge_frames: the (frames [n_frames, m, 4], tiles [n_frames, m]) pairs the ranks of one run returned from
    MultiSolver.track_frames(tiles=True), folded -> the pair of the whole run.  Host code; no GPU needed."""
    parts = [(np.ascontiguousarray(f, np.float32), np.ascontiguousarray(t, np.uint32)) for f, t in parts]
    if not parts:
        raise ValueError("track_merge_frames needs at least one part (the shape of the frames is the parts')")
    shape = parts[0][1].shape
    if any(t.shape != shape or f.shape != shape + (4,) for f, t in parts):
        raise ValueError("track_merge_frames: every part is (float32 [n_frames, m, 4], uint32 [n_frames, m]) of one shape")
    n = int(np.prod(shape))
    fp = (C.c_void_p * len(parts))(*[f.ctypes.data or 1 for f, _ in parts])
    tp = (C.c_void_p * len(parts))(*[t.ctypes.data or 1 for _, t in parts])
    out, til = np.zeros(shape + (4,), np.float32), np.zeros(shape, np.uint32)
    L = _lib.lib()
    rc = L.sphx_track_merge_frames(n, fp, tp, len(parts), out.ctypes.data or 1, til.ctypes.data or 1)
    if rc:
        raise SphxError(rc, L.sphx_multi_last_error(None).decode())
    return out, til


FIELD_NAMES = ("vel_grad", "divergence", "vorticity", "color_grad")
_FIELD_WIDTH = dict(vel_grad=4, divergence=1, vorticity=1, color_grad=2)  # floats per particle
_FIELD_SHAPE = dict(vel_grad=(2, 2), divergence=(), vorticity=(), color_grad=(2,))


def _field_names(fields):
    fields = (fields,) if isinstance(fields, str) else tuple(fields)
    bad = [f for f in fields if f not in FIELD_NAMES]
    if bad or not fields:
        raise ValueError("fields must be a non-empty subset of %s, not %r" % (FIELD_NAMES, fields))
    return fields


# one record of sphx_fluid_stats (sphx_stats_rec, 128 bytes) and one frame entry of the recorder (sphx_stats_frame, 16 bytes)
STATS_DTYPE = np.dtype([("count", "<u8"), ("nonfinite", "<u8"), ("density_count", "<u8"), ("density_valid", "<u4"), ("reserved", "<u4"),
                        ("sum_pos", "<f8", (2,)), ("sum_vel", "<f8", (2,)), ("sum_speed_sq", "<f8"), ("sum_angular", "<f8"),
                        ("sum_density", "<f8"), ("sum_density_sq", "<f8"), ("max_speed_sq", "<f8"), ("min_pos", "<f4", (2,)),
                        ("max_pos", "<f4", (2,)), ("min_density", "<f4"), ("max_density", "<f4")])
STATS_FRAME_DTYPE = np.dtype([("step", "<u8"), ("dt", "<f4"), ("n", "<u4")])


# a gauge (sphx_gauge: the ray x0 + k * dx, y0 + k * dy, 0 <= k < n), its record (sphx_gauge_rec) and a point probe of a recorded frame
# (sphx_probe_rec); 32 bytes each
GAUGE_DTYPE = np.dtype([("x0", "<f4"), ("y0", "<f4"), ("dx", "<f4"), ("dy", "<f4"), ("n", "<u4"), ("reserved", "<u4", (3,))])
GAUGE_REC_DTYPE = np.dtype([("first", "<u4"), ("last", "<u4"), ("inside", "<u4"), ("t", "<f4"), ("x", "<f4"), ("y", "<f4"), ("f_last", "<f4"),
                            ("f_next", "<f4")])
PROBE_REC_DTYPE = np.dtype([("density", "<f4"), ("fraction", "<f4"), ("velocity", "<f4", (2,)), ("count", "<u4"), ("reserved", "<u4", (3,))])
# what one tile of a tiled run knows of a gauge (sphx_gauge_part): the interval it owns and the reduction over it; 32 bytes
GAUGE_PART_DTYPE = np.dtype([("lo", "<u4"), ("count", "<u4"), ("first", "<u4"), ("last", "<u4"), ("inside", "<u4"), ("f_lo", "<f4"),
                             ("f_last", "<f4"), ("f_next", "<f4")])


def _gauge_array(gauges):
    """[g, 5] rows of x0, y0, dx, dy, n (or a GAUGE_DTYPE array, or None) -> contiguous GAUGE_DTYPE array [g]."""
    if gauges is None:
        return np.zeros(0, GAUGE_DTYPE)
    if isinstance(gauges, np.ndarray) and gauges.dtype == GAUGE_DTYPE:
        return np.ascontiguousarray(gauges).reshape(-1)
    a = np.asarray(gauges, np.float64)
    if a.size == 0:
        return np.zeros(0, GAUGE_DTYPE)
    if a.ndim == 1:
        a = a[None, :]
    if a.ndim != 2 or a.shape[1] != 5:
        raise ValueError("gauges must be [g, 5] rows of x0, y0, dx, dy, n or a GAUGE_DTYPE array, not shape %s" % (a.shape,))
    n = a[:, 4]
    if not (np.isfinite(n).all() and (n == np.floor(n)).all() and (n >= 0).all() and (n < 2.0 ** 32).all()):
        raise ValueError("the sample counts n of gauges must be whole numbers in [0, 2^32)")
    g = np.zeros(len(a), GAUGE_DTYPE)
    for k, name in enumerate(("x0", "y0", "dx", "dy")):
        g[name] = a[:, k].astype(np.float32)
    g["n"] = n.astype(np.uint32)
    return g


def gauge_reduce(values, gauges, iso=0.5):
    """sphx_gauge_reduce: the gauge rule of include/sphx.h over given values (float32, gauges[k].n per gauge, gauge after gauge) ->
    GAUGE_REC_DTYPE array [g].  Host code; no GPU.  The device (SphxContext.gauges) agrees with it bit for bit."""
    g = _gauge_array(gauges)
    v = np.ascontiguousarray(values, np.float32).reshape(-1)
    if len(v) != int(g["n"].astype(np.int64).sum()):
        raise ValueError("values must hold %d floats (the sum of the gauges' n), not %d" % (int(g["n"].astype(np.int64).sum()), len(v)))
    rec = np.zeros(len(g), GAUGE_REC_DTYPE)
    rc = _lib.lib().sphx_gauge_reduce(_p(v) if len(v) else None, _p(g) if len(g) else None, len(g), iso, _p(rec) if len(g) else rec.ctypes.data or 1)
    if rc:
        raise SphxError(rc, "sphx_gauge_reduce: invalid argument (see include/sphx.h, \"gauges and probes\")")
    return rec


def gauge_merge(parts, gauges, iso=0.5):
    """sphx_gauge_merge: fold the tiles' (or ranks') parts of MultiSolver.gauges(..., tiles=True) — GAUGE_PART_DTYPE arrays [g], a list of
    them or one array [p, g] — into the GAUGE_REC_DTYPE records [g] of `gauges` (the gauges and the iso of the calls that made the parts).
    Host code; no GPU.  The parts with samples must tile every gauge exactly: a gap, an overlap or a wrong count raises SphxError."""
    g = _gauge_array(gauges)
    ps = [np.ascontiguousarray(p, GAUGE_PART_DTYPE).reshape(-1, len(g)) for p in ([parts] if isinstance(parts, np.ndarray) else parts)]
    arr = np.ascontiguousarray(np.concatenate(ps, 0)) if ps else np.zeros((0, len(g)), GAUGE_PART_DTYPE)
    rec = np.zeros(len(g), GAUGE_REC_DTYPE)
    L = _lib.lib()
    rc = L.sphx_gauge_merge(_p(g) if len(g) else None, len(g), iso, _p(arr) if arr.size else None, len(arr), rec.ctypes.data or 1)
    if rc:
        raise SphxError(rc, L.sphx_multi_last_error(None).decode())
    return rec


SCENE_RECT = (-0.1, -0.1, 2.1, 1.6)  # the world rectangle the reference app's camera is fitted to (main.rs:137), at scale 1
_VIEW_FIELDS = ("width", "height", "center", "pixel_per_world_unit", "radius", "min_pixel_radius", "speed_scale", "background", "boundary")


def _set_view_fields(view, fields):
    for k, val in fields.items():
        if k not in _VIEW_FIELDS:
            raise TypeError("unknown view field %r (one of %s)" % (k, ", ".join(_VIEW_FIELDS)))
        if k in ("center", "background", "boundary"):
            val = tuple(val)
            if len(val) != len(getattr(view, k)):
                raise ValueError("%s takes %d values" % (k, len(getattr(view, k))))
            val = type(getattr(view, k))(*val)
        setattr(view, k, val)
    return view


def render_fit(width, height, world_rect=SCENE_RECT, **view_fields):
    """sphx_render_fit: the camera of Camera::center_around_world_rect (camera.rs:21-35) for a width x height screen and the world
    rectangle (x, y, w, h), with the reference app's drawing defaults, as a SphxRenderView; view_fields override single fields
    (radius, min_pixel_radius, speed_scale, background, boundary, center, pixel_per_world_unit).  Needs no GPU."""
    v = _lib.SphxRenderView()
    x, y, w, h = (float(t) for t in world_rect)
    rc = _lib.lib().sphx_render_fit(int(width), int(height), x, y, w, h, C.byref(v))
    if rc:
        raise SphxError(rc, "sphx_render_fit: world_rect must be finite with w, h > 0")
    return _set_view_fields(v, view_fields)


def render_merge(layers):
    """sphx_render_merge: the layers of MultiSolver.render_layer() (dicts of key, owner and optionally rgba, all of one view) folded in
    the order given into one such dict — per pixel fluid over boundary over nothing, and of two fluid owners the one whose cell has the
    greater Morton code (the composite rule of include/sphx.h, "picture of a tiled run").  rgba is merged iff every layer has it.  Pure
    host code: needs no GPU."""
    layers = list(layers)
    if not layers:
        raise ValueError("render_merge needs at least one layer (the size of the picture is the layers')")
    h, w = np.asarray(layers[0]["owner"]).shape
    rgba = all(l.get("rgba") is not None for l in layers)
    keep, arr = [], (_lib.SphxRenderLayer * len(layers))()
    for i, l in enumerate(layers):
        k, o = np.ascontiguousarray(l["key"], np.uint32), np.ascontiguousarray(l["owner"], np.uint32)
        c = np.ascontiguousarray(l["rgba"], np.uint8) if rgba else None
        if k.shape != (h, w) or o.shape != (h, w) or (rgba and c.shape != (h, w, 4)):
            raise ValueError("layer %d: key and owner must be (%d, %d), rgba (%d, %d, 4)" % (i, h, w, h, w))
        keep.append((k, o, c))
        arr[i] = _lib.SphxRenderLayer(k.ctypes.data or 1, o.ctypes.data or 1, (c.ctypes.data or 1) if rgba else None)
    out = dict(key=np.zeros((h, w), np.uint32), owner=np.zeros((h, w), np.uint32))
    if rgba:
        out["rgba"] = np.zeros((h, w, 4), np.uint8)
    o = _lib.SphxRenderLayer(out["key"].ctypes.data or 1, out["owner"].ctypes.data or 1, (out["rgba"].ctypes.data or 1) if rgba else None)
    L = _lib.lib()
    rc = L.sphx_render_merge(w, h, arr, len(layers), C.byref(o))
    if rc:
        raise SphxError(rc, L.sphx_multi_last_error(None).decode())
    return out


def _copy_view(view):
    v = _lib.SphxRenderView()
    C.memmove(C.byref(v), C.byref(view), C.sizeof(v))
    return v


def write_png(path, rgba):
    """Write a uint8 (H, W, 4) RGBA or (H, W, 3) RGB image as a PNG (8 bits per channel, filter 0 on every row; standard library only)."""
    import struct
    import zlib

    a = np.ascontiguousarray(rgba, np.uint8)
    if a.ndim != 3 or a.shape[2] not in (3, 4) or a.shape[0] == 0 or a.shape[1] == 0:
        raise ValueError("rgba must be a non-empty uint8 (H, W, 4) or (H, W, 3) array, not shape %s" % (a.shape,))
    h, w, ch = a.shape

    def chunk(kind, data):
        return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)

    rows = np.zeros((h, 1 + w * ch), np.uint8)  # one filter-type byte (0 = None) in front of every row
    rows[:, 1:] = a.reshape(h, w * ch)
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 6 if ch == 4 else 2, 0, 0, 0)) +
                chunk(b"IDAT", zlib.compress(rows.tobytes(), 6)) + chunk(b"IEND", b""))


def gauge_elevation(ctx, xs, y_lo, y_hi, dy, kernel=KERNEL_WENDLAND_C2):
    """Free-surface elevation at each gauge x (the water height of a dam-break gauge).

    For each x, `fraction` is sampled on a one-column lattice from y_lo in steps of dy: ny = floor((y_hi - y_lo) / dy) + 1 samples
    (float64 on the host), at the fp32 points y_k = fl(y_lo + fl(k * dy)).  k = the highest sample with fraction >= 0.5; the elevation is
    y_k if k is the top sample, else the float64 linear interpolation to 0.5 between samples k and k + 1; NaN where the column holds no
    such sample.  Returns a float64 array, one value per gauge."""
    ny = int(np.floor((float(y_hi) - float(y_lo)) / float(dy))) + 1
    if ny <= 0:
        raise ValueError("need y_hi >= y_lo and dy > 0")
    y = np.float32(y_lo) + np.arange(ny, dtype=np.float32) * np.float32(dy)
    out = []
    for x in np.atleast_1d(np.asarray(xs, np.float64)):
        f = ctx.sample_grid((np.float32(x), np.float32(y_lo)), (np.float32(1.0), np.float32(dy)), (ny, 1), kernel=kernel,
                            fields=("fraction",))["fraction"][:, 0]
        out.append(_elevation(y, f))
    return np.array(out, np.float64)


def contour_chain(segments):
    """sphx_contour_chain: (order [n], line_first [lines + 1], closed [lines]) of segments [n, 2, 2] (or [n, 4]): the segment indices
    line after line, where each line starts in `order`, and which lines are closed.  The rule is in include/sphx.h.  Host code; no GPU."""
    seg = np.ascontiguousarray(segments, np.float32).reshape(-1, 4)
    n = len(seg)
    order, first, closed, lines = np.zeros(n, np.uint32), np.zeros(n + 1, np.uint32), np.zeros(n, np.uint8), C.c_uint32()
    rc = _lib.lib().sphx_contour_chain(_p(seg), n, _p(order), _p(first), _p(closed), C.byref(lines))
    if rc:
        raise SphxError(rc, "sphx_contour_chain")
    return order, first[:lines.value + 1], closed[:lines.value].astype(bool)


def contour_lines(segments):
    """The polylines of a contour (SphxContext.contour()["segments"]): -> (list of float32 [k, 2] point arrays, list of closed flags).
    A line of s segments has k = s + 1 points: the start of its first segment and every segment's end (a closed line repeats its first
    point as its last).  Stitched by sphx_contour_chain; host code, no GPU."""
    seg = np.ascontiguousarray(segments, np.float32).reshape(-1, 2, 2)
    order, first, closed = contour_chain(seg)
    lines = []
    for k in range(len(closed)):
        idx = order[first[k]:first[k + 1]]
        lines.append(np.concatenate([seg[idx[:1], 0], seg[idx, 1]]))
    return lines, [bool(c) for c in closed]


def contour_merge(parts, cap=None):
    """sphx_contour_merge: the parts the ranks of one run returned from MultiSolver.contour() (dicts with "segments", "cell", "count" and
    optionally "tile") folded into the contour of the whole run by a stable merge on the cell word -> dict(segments [n, 2, 2], cell [n],
    count, and tile [n] if every part has one).  cap: the most segments to return (None: all).  A part that holds fewer entries than
    its count raises SphxError(ERR_CAPACITY); its .count is the total to ask every rank for.  contour_lines() takes the result's
    segments as they are.  Host code; no GPU."""
    parts = list(parts)
    with_tile = bool(parts) and all("tile" in p for p in parts)
    kept = []
    arr = (_lib.SphxMultiContourOut * max(len(parts), 1))()
    stored = np.zeros(max(len(parts), 1), np.uint32)
    for k, p in enumerate(parts):
        seg = np.ascontiguousarray(p["segments"], np.float32).reshape(-1, 4)
        cel = np.ascontiguousarray(p["cell"], np.uint32)
        cnt = np.array([p["count"]], np.uint32)
        til = np.ascontiguousarray(p["tile"], np.int32) if with_tile else None
        if len(cel) != len(seg) or (til is not None and len(til) != len(seg)):
            raise ValueError("contour_merge: the arrays of a part differ in length")
        kept.append((seg, cel, cnt, til))
        stored[k] = len(seg)
        arr[k].segments, arr[k].cell, arr[k].count = seg.ctypes.data or 1, cel.ctypes.data or 1, cnt.ctypes.data
        arr[k].tile = (til.ctypes.data or 1) if with_tile else None
    cap_ = int(sum(int(s) for s in stored[:len(parts)])) if cap is None else int(cap)
    seg, cel, til = np.zeros((cap_, 2, 2), np.float32), np.zeros(cap_, np.uint32), np.full(cap_, -1, np.int32)
    cnt = np.zeros(1, np.uint32)
    o = _lib.SphxMultiContourOut()
    o.segments, o.cell, o.count = seg.ctypes.data or 1, cel.ctypes.data or 1, cnt.ctypes.data
    o.tile = (til.ctypes.data or 1) if with_tile else None
    L = _lib.lib()
    rc = L.sphx_contour_merge(arr, stored.ctypes.data_as(C.POINTER(C.c_uint32)), len(parts), cap_, C.byref(o))
    if rc:
        e = SphxError(rc, L.sphx_multi_last_error(None).decode())
        e.count = int(cnt[0])
        raise e
    count = int(cnt[0])
    n = min(count, cap_)
    res = dict(segments=seg[:n], cell=cel[:n], count=count)
    if with_tile:
        res["tile"] = til[:n]
    return res


_QUERY_ENTRY = (("id", np.uint32), ("dist_sq", np.float32), ("slot", np.uint32))
_QUERY_POINT = (("nearest_id", np.uint32), ("nearest_slot", np.uint32), ("nearest_dist_sq", np.float32))


def query_merge(parts, cap=None):
    """sphx_query_merge: the parts the ranks of one run returned from MultiSolver.query() for the SAME points (dicts with "offsets",
    "tile", "count" and the lists / nearest arrays) folded into the answer of the whole run in the caller's point order -> a dict like
    MultiSolver.query(tiles=True)'s, with the arrays every part has.  Per point the part with tile >= 0 answers (the lowest tile if
    several do); nobody: an empty range, tile -1.  cap: the most entries to return (None: all).  A part that holds fewer entries than
    the result needs raises SphxError(ERR_CAPACITY).  Host code; no GPU."""
    parts = list(parts)
    if not parts:
        raise ValueError("query_merge: no parts (the number of points is taken from them)")
    m = len(parts[0]["offsets"]) - 1
    entry = [(f, t) for f, t in _QUERY_ENTRY if all(f in p for p in parts)]
    point = [(f, t) for f, t in _QUERY_POINT if all(f in p for p in parts)]
    arr = (_lib.SphxMultiQueryOut * len(parts))()
    held = np.zeros(len(parts), np.uint64)
    keep = []
    for k, p in enumerate(parts):
        off = np.ascontiguousarray(p["offsets"], np.uint64)
        til = np.ascontiguousarray(p["tile"], np.int32)
        if len(off) != m + 1 or len(til) != m:
            raise ValueError("query_merge: the parts answer different point sets")
        keep += [off, til]
        arr[k].offsets, arr[k].tile = off.ctypes.data, til.ctypes.data or 1
        for f, t in entry + point:
            a = np.ascontiguousarray(p[f], t)
            keep.append(a)
            setattr(arr[k], f, a.ctypes.data or 1)
        held[k] = min(len(p[f]) for f, _ in entry) if entry else 0
    cap_ = sum(int(p["offsets"][m]) for p in parts) if cap is None else int(cap)  # (None: an upper bound, the parts' totals together)
    res = dict(offsets=np.zeros(m + 1, np.uint64), tile=np.full(m, -1, np.int32))
    res.update({f: np.zeros(cap_, t) for f, t in entry})
    res.update({f: np.zeros(m, t) for f, t in point})
    cnt = np.zeros(1, np.uint64)
    o = _lib.SphxMultiQueryOut()
    o.count = cnt.ctypes.data
    for f, a in res.items():
        setattr(o, f, a.ctypes.data or 1)
    L = _lib.lib()
    rc = L.sphx_query_merge(m, arr, held.ctypes.data_as(C.POINTER(C.c_uint64)), len(parts), cap_, C.byref(o))
    if rc:
        raise SphxError(rc, L.sphx_multi_last_error(None).decode())
    n = min(int(cnt[0]), cap_)
    for f, _ in entry:
        res[f] = res[f][:n]
    res["count"] = int(cnt[0])
    return res


def _elevation(y, f):
    wet = np.nonzero(f >= np.float32(0.5))[0]
    if len(wet) == 0:
        return float("nan")
    k = int(wet[-1])
    if k == len(f) - 1:
        return float(y[k])
    fk, fk1 = float(f[k]), float(f[k + 1])
    return float(y[k]) + (fk - 0.5) / (fk - fk1) * (float(y[k + 1]) - float(y[k]))


def _rect_array(rects):
    """One (x0, y0, x1, y1) tuple or a sequence of them -> (SphxRect array or None, count)."""
    r = np.asarray(rects, np.float32)
    if r.size == 0:
        return None, 0
    if r.ndim == 1:
        r = r[None, :]
    if r.ndim != 2 or r.shape[1] != 4:
        raise ValueError("rects must be one (x0, y0, x1, y1) tuple or a sequence of them, not shape %s" % (r.shape,))
    arr = (_lib.SphxRect * len(r))(*[_lib.SphxRect(*(float(v) for v in row)) for row in r])
    return arr, len(r)


def _append_arrays(pos, vel):
    pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 2)
    if vel is not None:
        vel = np.ascontiguousarray(vel, np.float32).reshape(-1, 2)
        if len(vel) != len(pos):
            raise ValueError("vel must have one row per row of pos")
    return pos, vel


class SphxContext:
    """Device solver context (sphx_ctx).  Mirrors DFSPHSolver + the solver-owned part of FluidParticleWorld."""

    def __init__(self, params=None, **kw):
        self.L = _lib.lib()
        self.params = params if params is not None else default_params(**kw)
        h = C.c_void_p()
        rc = self.L.sphx_create(C.byref(self.params), C.byref(h))
        if rc:
            raise SphxError(rc, self.L.sphx_last_error(None).decode())
        self.h = h

    def close(self):
        if getattr(self, "h", None) and getattr(self, "_owned", True):
            self.L.sphx_destroy(self.h)
        self.h = None

    __del__ = close

    def _chk(self, rc):
        if rc:
            raise SphxError(rc, self.L.sphx_last_error(self.h).decode())

    @property
    def n(self):
        return self.L.sphx_num_particles(self.h)

    @property
    def nb(self):
        return self.L.sphx_num_boundary(self.h)

    def set_boundary(self, xy):
        xy = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
        self._chk(self.L.sphx_set_boundary(self.h, _p(xy), len(xy)))

    def upload(self, pos, vel=None):
        pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 2)
        if vel is not None:
            vel = np.ascontiguousarray(vel, np.float32).reshape(-1, 2)
        self._chk(self.L.sphx_upload(self.h, _p(pos), _p(vel), len(pos)))

    def append(self, pos, vel=None):
        """sphx_append: add particles behind the present ones on the device (vel None = zero) -> the id of the first new particle."""
        pos, vel = _append_arrays(pos, vel)
        first = C.c_uint32()
        self._chk(self.L.sphx_append(self.h, _p(pos), _p(vel), len(pos), C.byref(first)))
        return first.value

    def remove(self, rects, outside=False):
        """sphx_remove: drop the particles inside any of the rectangles (one (x0, y0, x1, y1) tuple or a sequence of them, half-open,
        bounds may be infinite) — with outside=True those inside none of them (a keep-box) -> the number removed."""
        arr, k = _rect_array(rects)
        removed = C.c_uint32()
        self._chk(self.L.sphx_remove(self.h, arr, k, _lib.REMOVE_OUTSIDE if outside else 0, C.byref(removed)))
        return removed.value

    def clear_cached(self):
        self._chk(self.L.sphx_clear_cached(self.h))

    def step_begin(self, dt_prev, law=None):
        """Phase A.  law (TimeManager.law(diameter)): the device derives dt itself and starts phase B without waiting for the
        host (sphx_step_begin_law); step_finish then verifies the host's dt against it."""
        v = C.c_float()
        if law is None:
            self._chk(self.L.sphx_step_begin(self.h, dt_prev, C.byref(v)))
        else:
            self._chk(self.L.sphx_step_begin_law(self.h, dt_prev, C.byref(law), C.byref(v)))
        return v.value

    def step_finish(self, dt):
        st = SphxStepStats()
        self._chk(self.L.sphx_step_finish(self.h, dt, C.byref(st)))
        return st.as_dict()

    def view_request(self, stride=1):
        """Start an asynchronous strided download of {x, y, |v|} (the viewer's per-frame data, main.rs:239-258)."""
        n = C.c_uint32()
        self._chk(self.L.sphx_view_request(self.h, stride, C.byref(n)))
        return n.value

    def view_fetch(self, wait=True):
        """-> float32 array [count, 3] (a copy of the pinned buffer), or None if wait=False and the copy is still in flight."""
        ptr, n = C.POINTER(C.c_float)(), C.c_uint32()
        rc = self.L.sphx_view_fetch(self.h, int(wait), C.byref(ptr), C.byref(n))
        if rc == _lib.ERR_NOT_READY and not wait:
            return None
        self._chk(rc)
        if n.value == 0:
            return np.zeros((0, 3), np.float32)
        return np.ctypeslib.as_array(ptr, shape=(n.value, 3)).copy()

    def wcsph_step_begin(self, dt):
        """WCSPHSolver::simulation_step up to the timer call (wscsph.rs:126-161) -> vmax."""
        v = C.c_float()
        self._chk(self.L.sphx_wcsph_step_begin(self.h, dt, C.byref(v)))
        return v.value

    def wcsph_step_finish(self, dt):
        st = SphxStepStats()
        self._chk(self.L.sphx_wcsph_step_finish(self.h, dt, C.byref(st)))
        return st.as_dict()

    def update_neighborhood(self):
        self._chk(self.L.sphx_update_neighborhood(self.h))

    def update_densities(self, kind=KERNEL_WENDLAND_C2):
        self._chk(self.L.sphx_update_densities(self.h, kind))

    def compute_alpha(self):
        self._chk(self.L.sphx_compute_alpha(self.h))

    def synchronize(self):
        self._chk(self.L.sphx_synchronize(self.h))

    def set_tiling_invariant(self, on=True):
        """sphx_set_tiling_invariant: cell mates ordered by persistent id, warm-start values travel with their particle (a comparison
        mode for multi-GPU runs; not the reference's behaviour)."""
        self._chk(self.L.sphx_set_tiling_invariant(self.h, int(bool(on))))

    def download(self, pos=True, vel=True, density=True, ids=True):
        n = self.n
        out = {}
        a_pos = np.zeros((n, 2), np.float32) if pos else None
        a_vel = np.zeros((n, 2), np.float32) if vel else None
        a_den = np.zeros(n, np.float32) if density else None
        a_ids = np.zeros(n, np.uint32) if ids else None
        self._chk(self.L.sphx_download(self.h, _p(a_pos), _p(a_vel), _p(a_den), _p(a_ids)))
        out.update(pos=a_pos, vel=a_vel, density=a_den, ids=a_ids)
        return out

    # ---- following particles by id (the contract is in include/sphx.h, "following particles by id") ----
    def track(self, ids):
        """sphx_track_set: the ids to follow (any order, duplicates allowed, at most _lib.TRACK_MAX_IDS; an empty sequence clears the
        set).  Discards a recording."""
        ids = np.ascontiguousarray(ids, np.uint32).reshape(-1)
        self._chk(self.L.sphx_track_set(self.h, _p(ids) if len(ids) else None, len(ids)))

    def track_status(self):
        """sphx_track_get_status -> dict(m, recording, max_frames, every, frames, dropped)."""
        st = _lib.SphxTrackStatus()
        self._chk(self.L.sphx_track_get_status(self.h, C.byref(st)))
        return {k: getattr(st, k) for k, _ in st._fields_ if k != "reserved"}

    def track_fetch(self, out=None, fields=TRACK_FIELDS):
        """sphx_track_fetch: where the tracked particles are now, in the order of track(ids), without a download of the arrays.

        out=None: returns {"slot": uint32 [m], "pos": float32 [m, 2], "vel": float32 [m, 2], "density": float32 [m]} (the requested
        `fields`) as numpy arrays.  An id no particle carries has slot _lib.TRACK_ABSENT and NaN records (the word 0x7FC00000).
        out={field: torch tensor on the context's device} (contiguous; slot int32, the others float32; the sizes above) selects the
        device path: the library writes into the tensors on its own stream; torch's current stream is synchronised before the call
        and the context's stream after it, as in sample().  Returns out."""
        m = self.track_status()["m"]
        if out is not None:
            import torch

            o = _lib.SphxTrackOut()
            for f, t in out.items():
                want = m * (2 if f in ("pos", "vel") else 1)
                if f not in TRACK_FIELDS or not _is_torch(t) or t.device.type != "cuda" or not t.is_contiguous() or t.numel() != want or \
                        t.dtype != (torch.int32 if f == "slot" else torch.float32):
                    raise ValueError("out[%r] must be a contiguous %s cuda tensor of %d elements" % (f, "int32" if f == "slot" else "float32", want))
                setattr(o, f, t.data_ptr() or 1)
            torch.cuda.current_stream().synchronize()
            self._chk(self.L.sphx_track_fetch(self.h, _lib.TRACK_DEVICE_POINTERS, C.byref(o)))
            self.synchronize()
            return out
        outs = _track_outputs(fields, m)
        self._chk(self.L.sphx_track_fetch(self.h, 0, C.byref(_track_struct(outs))))
        return outs

    def fields(self, fields=FIELD_NAMES, out=None):
        """sphx_particle_fields: the velocity gradient, its divergence and vorticity, and the colour-field gradient at every particle, from
        the solver's own neighbour lists (the contract is in include/sphx.h).  Device order: row i belongs to row i of download().

        out=None: returns {name: numpy float32 array} for the requested `fields` — "vel_grad" [n, 2, 2] (d v_a / d x_b at [a, b]),
        "divergence" [n], "vorticity" [n], "color_grad" [n, 2].  color_grad is ~0 in the bulk and points into the fluid at a free
        surface (|color_grad| * h of order 1 there): a free-surface indicator and, negated and normalised, the surface normal.
        out={name: torch tensor on the context's device} (contiguous float32, the sizes above) selects the device path: the library
        writes into the tensors on its own stream; torch's current stream is synchronised before the call and the context's stream
        after it, as in track_fetch().  Returns out.
        Allowed where sample() is: after a finished step, or update_neighborhood() + update_densities()."""
        n = self.n
        if out is not None:
            import torch

            o = _lib.SphxFieldsOut()
            for f, t in out.items():
                want = n * _FIELD_WIDTH.get(f, 0)
                if f not in FIELD_NAMES or not _is_torch(t) or t.device.type != "cuda" or not t.is_contiguous() or t.numel() != want or \
                        t.dtype != torch.float32:
                    raise ValueError("out[%r] must be a contiguous float32 cuda tensor of %d elements" % (f, want))
                setattr(o, f, t.data_ptr() or 1)  # (an empty tensor has no storage: a non-NULL dummy still names the field; nothing is written)
            torch.cuda.current_stream().synchronize()
            self._chk(self.L.sphx_particle_fields(self.h, _lib.FIELDS_DEVICE_POINTERS, C.byref(o)))
            self.synchronize()
            return out
        outs = {f: np.zeros((n,) + _FIELD_SHAPE[f], np.float32) for f in _field_names(fields)}
        o = _lib.SphxFieldsOut()
        for f, a in outs.items():
            setattr(o, f, a.ctypes.data or 1)
        self._chk(self.L.sphx_particle_fields(self.h, 0, C.byref(o)))
        return outs

    # ---- fluid statistics (the contract is in include/sphx.h, "fluid statistics") ----
    def stats(self, rects=(), out=None):
        """sphx_fluid_stats: counts, float64 sums and exact extremes of the whole fluid (record 0) and of the particles inside each of up
        to _lib.STATS_MAX_RECTS rectangles (record 1 + k; (x0, y0, x1, y1) tuples, half-open, bounds may be infinite), from one
        streaming pass on the device.

        out=None: returns a numpy structured array [1 + len(rects)] of STATS_DTYPE.
        out=a contiguous torch uint8 tensor of (1 + len(rects)) * 128 bytes on the context's device selects the device path: the
        library writes the records into it on its own stream; torch's current stream is synchronised before the call and the
        context's stream after it, as in track_fetch().  Returns out (out.cpu().numpy().view(STATS_DTYPE) reads it).
        Momentum = m * sum_vel, E_kin = m / 2 * sum_speed_sq, E_pot = -m * (g . sum_pos)."""
        arr, k = _rect_array(rects)
        if out is not None:
            import torch

            if not _is_torch(out) or out.device.type != "cuda" or not out.is_contiguous() or out.dtype != torch.uint8 or \
                    out.numel() != (1 + k) * STATS_DTYPE.itemsize:
                raise ValueError("out must be a contiguous uint8 cuda tensor of %d bytes" % ((1 + k) * STATS_DTYPE.itemsize))
            torch.cuda.current_stream().synchronize()
            self._chk(self.L.sphx_fluid_stats(self.h, arr, k, _lib.STATS_DEVICE_POINTERS, out.data_ptr()))
            self.synchronize()
            return out
        rec = np.zeros(1 + k, STATS_DTYPE)
        self._chk(self.L.sphx_fluid_stats(self.h, arr, k, 0, _p(rec)))
        return rec

    def stats_record(self, rects, max_frames, every=1):
        """sphx_stats_record: from now on every `every`-th finished step stores one frame of stats(rects) on the device, up to max_frames
        frames (later ones are counted in stats_status()["dropped"]); max_frames=0 stops and frees.  Nothing is synchronised."""
        arr, k = _rect_array(rects)
        self._chk(self.L.sphx_stats_record(self.h, arr, k, max_frames, every))

    def stats_status(self):
        """sphx_stats_get_status -> dict(n_rects, recording, max_frames, every, frames, dropped)."""
        st = _lib.SphxStatsStatus()
        self._chk(self.L.sphx_stats_get_status(self.h, C.byref(st)))
        return {k: getattr(st, k) for k, _ in st._fields_ if k != "reserved"}

    def stats_frames(self, first=0, count=None):
        """sphx_stats_read -> (records [count, 1 + n_rects] of STATS_DTYPE, info [count] of STATS_FRAME_DTYPE: step, dt, n) for the
        recorded frames [first, first + count) (count=None: all from `first`).  Waits for the context's stream."""
        st = self.stats_status()
        if count is None:
            count = max(st["frames"] - first, 0)
        rec = np.zeros((count, 1 + st["n_rects"]), STATS_DTYPE)
        info = np.zeros(count, STATS_FRAME_DTYPE)
        self._chk(self.L.sphx_stats_read(self.h, first, count, _p(rec) if count else None, _p(info) if count else None))
        return rec, info

    # ---- gauges and probes (the contract is in include/sphx.h, "gauges and probes") ----
    def gauges(self, gauges, iso=0.5, field="fraction", kernel=KERNEL_WENDLAND_C2, values=False, out=None):
        """sphx_gauge_levels: each gauge is a ray of n samples, (x0 + k * dx, y0 + k * dy); its record names the lowest and the highest
        sample with field >= iso, their number, and the crossing point behind the highest one (a vertical gauge: the water level; a
        gauge with dy == 0: the front along the bed).

        gauges: [g, 5] rows of x0, y0, dx, dy, n, or a GAUGE_DTYPE array.  field: "fraction" or "density".
        Returns a GAUGE_REC_DTYPE array [g]; with values=True the pair (records, float32 values [sum n], gauge after gauge).
        Device path: out = a contiguous torch uint8 tensor of g * 32 bytes on the context's device, and values may be a float32 tensor
        of sum n values there; the library writes into them on its own stream (torch's current stream is synchronised before the call
        and the context's stream after it, as in stats()).  Returns out, or (out, values)."""
        if field not in _lib.GAUGE_FIELDS:
            raise ValueError("field must be one of %s, not %r" % (sorted(_lib.GAUGE_FIELDS), field))
        g = _gauge_array(gauges)
        total = int(g["n"].astype(np.int64).sum())
        gp = _p(g) if len(g) else None
        if out is not None:
            import torch

            if not _is_torch(out) or out.device.type != "cuda" or not out.is_contiguous() or out.dtype != torch.uint8 or \
                    out.numel() != len(g) * GAUGE_REC_DTYPE.itemsize:
                raise ValueError("out must be a contiguous uint8 cuda tensor of %d bytes" % (len(g) * GAUGE_REC_DTYPE.itemsize))
            val = values if _is_torch(values) else None
            if values is not False and values is not None and val is None:
                raise ValueError("with a device out, values must be a float32 cuda tensor of %d values (or False)" % total)
            if val is not None and (val.device.type != "cuda" or not val.is_contiguous() or val.dtype != torch.float32 or val.numel() != total):
                raise ValueError("values must be a contiguous float32 cuda tensor of %d values" % total)
            torch.cuda.current_stream(out.device).synchronize()
            self._chk(self.L.sphx_gauge_levels(self.h, gp, len(g), kernel, _lib.GAUGE_FIELDS[field], iso, _lib.GAUGE_DEVICE_POINTERS,
                                               out.data_ptr() or 1, (val.data_ptr() or 1) if val is not None else None))
            self.synchronize()
            return out if val is None else (out, val)
        rec = np.zeros(len(g), GAUGE_REC_DTYPE)
        val = np.zeros(total, np.float32) if values else None
        self._chk(self.L.sphx_gauge_levels(self.h, gp, len(g), kernel, _lib.GAUGE_FIELDS[field], iso, 0, rec.ctypes.data or 1,
                                           (val.ctypes.data or 1) if values else None))
        return (rec, val) if values else rec

    def probe_record(self, points=None, gauges=None, max_frames=0, every=1, iso=0.5, field="fraction", kernel=KERNEL_WENDLAND_C2):
        """sphx_probe_record: from now on every `every`-th finished step stores one frame on the device — sample(points)' four fields
        at the fixed points and the records of gauges(gauges, iso, field, kernel) — up to max_frames frames (later ones are counted in
        probe_status()["dropped"]); max_frames=0 stops and frees.  Nothing is synchronised."""
        if field not in _lib.GAUGE_FIELDS:
            raise ValueError("field must be one of %s, not %r" % (sorted(_lib.GAUGE_FIELDS), field))
        g = _gauge_array(gauges)
        pts = np.zeros((0, 2), np.float32) if points is None else np.ascontiguousarray(points, np.float32)
        if pts.ndim != 2 or pts.shape[1] != 2:
            raise ValueError("points must be a float32 [m, 2] array, not shape %s" % (pts.shape,))
        self._chk(self.L.sphx_probe_record(self.h, _p(pts) if len(pts) else None, len(pts), _p(g) if len(g) else None, len(g), kernel,
                                           _lib.GAUGE_FIELDS[field], iso, max_frames, every))

    def probe_status(self):
        """sphx_probe_get_status -> dict(m_points, n_gauges, recording, max_frames, every, frames, dropped)."""
        st = _lib.SphxProbeStatus()
        self._chk(self.L.sphx_probe_get_status(self.h, C.byref(st)))
        return {k: getattr(st, k) for k, _ in st._fields_ if k != "reserved"}

    def probe_frames(self, first=0, count=None):
        """sphx_probe_read -> dict(points [count, m_points] of PROBE_REC_DTYPE, gauges [count, n_gauges] of GAUGE_REC_DTYPE, info [count]
        of STATS_FRAME_DTYPE: step, dt, n) for the recorded frames [first, first + count) (count=None: all from `first`).  Waits for
        the context's stream."""
        st = self.probe_status()
        if count is None:
            count = max(st["frames"] - first, 0)
        pts = np.zeros((count, st["m_points"]), PROBE_REC_DTYPE)
        gau = np.zeros((count, st["n_gauges"]), GAUGE_REC_DTYPE)
        info = np.zeros(count, STATS_FRAME_DTYPE)
        self._chk(self.L.sphx_probe_read(self.h, first, count, _p(pts) if pts.size else None, _p(gau) if gau.size else None,
                                         _p(info) if count else None))
        return dict(points=pts, gauges=gau, info=info)

    def tile_stats(self, rects=()):
        """sphx_tile_fluid_stats: stats() of a TILE context (MultiSolver.tile_context(k)) over the particles that tile owns — its ghosts
        enter nothing.  A plain context is refused.  MultiSolver.stats() folds these over the tiles."""
        arr, k = _rect_array(rects)
        rec = np.zeros(1 + k, STATS_DTYPE)
        self._chk(self.L.sphx_tile_fluid_stats(self.h, arr, k, 0, _p(rec)))
        return rec

    def tile_render_layer(self, view=None, device=False, **view_fields):
        """sphx_tile_render_layer (a TILE context only: MultiSolver.tile_context(k)) -> dict(key, owner, rgba): the layer of the particles
        this tile owns and of the boundary particles of its cells, at the full size of the view (include/sphx.h, "picture of a tiled
        run").  device=True: the arrays are torch tensors on the context's device (key and owner int32: torch has no uint32 arithmetic),
        written through SPHX_RENDER_DEVICE_POINTERS.  A plain context is refused.  MultiSolver.render_layer() merges these."""
        from .multi import MultiSolver

        view = MultiSolver._view(view, view_fields)
        h, w = view.height, view.width
        if device:
            import torch

            dev = torch.device("cuda", torch.cuda.current_device())
            out = dict(key=torch.zeros((h, w), dtype=torch.int32, device=dev), owner=torch.zeros((h, w), dtype=torch.int32, device=dev),
                       rgba=torch.zeros((h, w, 4), dtype=torch.uint8, device=dev))
            o = _lib.SphxRenderLayer(*[(out[k].data_ptr() or 1) for k in ("key", "owner", "rgba")])
            torch.cuda.current_stream(dev).synchronize()
            self._chk(self.L.sphx_tile_render_layer(self.h, C.byref(view), _lib.RENDER_DEVICE_POINTERS, C.byref(o)))
            self.synchronize()
            return out
        out = dict(key=np.zeros((h, w), np.uint32), owner=np.zeros((h, w), np.uint32), rgba=np.zeros((h, w, 4), np.uint8))
        o = _lib.SphxRenderLayer(*[(out[k].ctypes.data or 1) for k in ("key", "owner", "rgba")])
        self._chk(self.L.sphx_tile_render_layer(self.h, C.byref(view), 0, C.byref(o)))
        return out

    def track_record(self, max_frames, every=1):
        """sphx_track_record: from now on every `every`-th finished step stores {x, y, vx, vy} of the tracked ids on the device, up to
        max_frames frames (later ones are counted in track_status()["dropped"]); max_frames=0 stops and frees.  Works inside
        DFSPHSolver.simulation_steps(k) too: the frames are taken behind each step's kernels, nothing is synchronised."""
        self._chk(self.L.sphx_track_record(self.h, max_frames, every))

    def track_frames(self, first=0, count=None):
        """sphx_track_read -> float32 [count, m, 4] = x, y, vx, vy of the recorded frames [first, first + count) (count=None: all from
        `first`).  Waits for the context's stream."""
        st = self.track_status()
        if count is None:
            count = max(st["frames"] - first, 0)
        out = np.zeros((count, st["m"], 4), np.float32)
        self._chk(self.L.sphx_track_read(self.h, first, count, 0, _p(out) if out.size else None))
        return out

    def ids_issued(self):
        """The number of ids handed out since the last upload (the id the next append() would start from); 0 before any upload."""
        first = C.c_uint32()
        rc = self.L.sphx_append(self.h, None, None, 0, C.byref(first))  # (m == 0: a no-op that reports the next id)
        if rc == _lib.ERR_NOT_READY:
            return 0
        self._chk(rc)
        return first.value

    def download_by_id(self, first=0, count=None, fields=TRACK_FIELDS):
        """sphx_download_by_id: the particles with the ids first .. first + count - 1 in id order (count=None: up to the ids issued so
        far) -> the dict of track_fetch() plus "present", the number of ids found.  After an unedited upload download_by_id() is the
        particles in upload order, whatever the steps since."""
        if count is None:
            count = max(self.ids_issued() - first, 0)
        outs = _track_outputs(fields, count)
        present = C.c_uint32()
        self._chk(self.L.sphx_download_by_id(self.h, first, count, 0, C.byref(_track_struct(outs)), C.byref(present)))
        outs["present"] = present.value
        return outs

    def download_boundary(self):
        xy = np.zeros((self.nb, 2), np.float32)
        ids = np.zeros(self.nb, np.uint32)
        self._chk(self.L.sphx_download_boundary(self.h, _p(xy), _p(ids)))
        return xy, ids

    def download_solver_state(self):
        n = self.n
        a, k, s = (np.zeros(n, np.float32) for _ in range(3))
        self._chk(self.L.sphx_download_solver_state(self.h, _p(a), _p(k), _p(s)))
        return dict(alpha=a, kappa=k, stiffness=s)

    def download_neighbors(self):
        """-> (counts[N,2] u16 (dynamic,total), start[N+1] u64, lists u32) in the canonical form of sphx.h."""
        n = self.n
        counts = np.zeros((n, 2), np.uint16)
        total = C.c_uint64()
        self._chk(self.L.sphx_download_neighbors(self.h, _p(counts), None, C.byref(total)))
        lists = np.zeros(total.value, np.uint32)
        self._chk(self.L.sphx_download_neighbors(self.h, None, _p(lists), C.byref(total)))
        start = np.zeros(n + 1, np.uint64)
        np.cumsum(counts[:, 1].astype(np.uint64), out=start[1:])
        return counts, start, lists

    def download_cells(self, static=False):
        m = C.c_uint32()
        self._chk(self.L.sphx_download_cells(self.h, int(static), None, None, C.byref(m)))
        first = np.zeros(m.value, np.uint32)
        cidx = np.zeros(m.value, np.uint32)
        self._chk(self.L.sphx_download_cells(self.h, int(static), _p(first), _p(cidx), C.byref(m)))
        return first, cidx

    def last_flags(self):
        return self.L.sphx_last_flags(self.h)

    def correction_counts(self):
        """sphx_debug_correction_counts -> (skipped, stopped by a window flag, stopped by a remote entry): cumulative correction
        workgroups of a context created with SPHX_ZERO_SKIP_COUNT=1 in the environment (all zero otherwise)."""
        out = (C.c_uint64 * 3)()
        self._chk(self.L.sphx_debug_correction_counts(self.h, out))
        return int(out[0]), int(out[1]), int(out[2])

    def quiet_counts(self):
        """sphx_debug_quiet_counts -> (workgroups that left through the quiet-scene exit, corrections queued in the decide-first
        form): cumulative, of a context created with SPHX_ZERO_SKIP_COUNT=1 in the environment (all zero otherwise)."""
        out = (C.c_uint64 * 2)()
        self._chk(self.L.sphx_debug_quiet_counts(self.h, out))
        return int(out[0]), int(out[1])

    def takeover_counts(self):
        """sphx_debug_takeover_counts -> (corrections queued in the thin form, producers that also stored the warm-start sums,
        particles whose cell a recount moved — always 0): cumulative since the context was created."""
        out = (C.c_uint64 * 3)()
        self._chk(self.L.sphx_debug_takeover_counts(self.h, out))
        return int(out[0]), int(out[1]), int(out[2])

    def rigid_counts(self):
        """sphx_debug_rigid_counts -> (non-pressure passes queued in the rigid form, those that found no mark and stored the uniform
        acceleration, those that found a mark and ran the full pass): cumulative since the context was created."""
        out = (C.c_uint64 * 3)()
        self._chk(self.L.sphx_debug_rigid_counts(self.h, out))
        return int(out[0]), int(out[1]), int(out[2])

    def rigid_predict_counts(self):
        """sphx_debug_rigid_predict_counts -> (first density producers queued in the rigid form, workgroups that took the fluid-only
        exit, workgroups that walked with the uniform acceleration, launches that found no verdict); the last three are counted with
        SPHX_ZERO_SKIP_COUNT=1 only.  Cumulative since the context was created."""
        out = (C.c_uint64 * 4)()
        self._chk(self.L.sphx_debug_rigid_predict_counts(self.h, out))
        return int(out[0]), int(out[1]), int(out[2]), int(out[3])

    def download_accel(self):
        """sphx_debug_download_accel -> float32 [N, 2]: accel[] as the latest non-pressure pass left it (sorted order)."""
        out = np.zeros((self.n, 2), np.float32)
        self._chk(self.L.sphx_debug_download_accel(self.h, out.ctypes.data_as(C.c_void_p)))
        return out

    def download_wcsph_half_step(self):
        """sphx_debug_download_wcsph_half_step -> download()'s dictionary between wcsph_step_begin and wcsph_step_finish: the
        leap-frogged positions, the velocities at the half step, the Poly6 densities and the ids (sorted order)."""
        n = self.n
        out = dict(pos=np.zeros((n, 2), np.float32), vel=np.zeros((n, 2), np.float32), density=np.zeros(n, np.float32), ids=np.zeros(n, np.uint32))
        self._chk(self.L.sphx_debug_download_wcsph_half_step(self.h, _p(out["pos"]), _p(out["vel"]), _p(out["density"]), _p(out["ids"])))
        return out

    def grid_info(self, which=0):
        """Cell table behind the grid: covered blocks, table entries, directory extent (sphx_grid_info)."""
        out = (C.c_uint32 * 4)()
        self._chk(self.L.sphx_grid_info(self.h, which, out))
        return dict(blocks=out[0], entries=out[1], nbx=out[2], nby=out[3])

    def constants(self):
        out = np.zeros(6, np.float32)
        self._chk(self.L.sphx_get_constants(self.h, _p(out)))
        return out

    def viscosity(self):
        """sphx_get_viscosity: (model name, fluid_viscosity, normalizer_laplacian) the context runs."""
        m, mu, nlap = C.c_uint32(), C.c_float(), C.c_float()
        self._chk(self.L.sphx_get_viscosity(self.h, C.byref(m), C.byref(mu), C.byref(nlap)))
        return {VISCOSITY_XSPH: "xsph", VISCOSITY_PHYSICAL: "physical"}[m.value], np.float32(mu.value), np.float32(nlap.value)

    def sample(self, points, kernel=KERNEL_WENDLAND_C2, fields=SAMPLE_FIELDS):
        """sphx_sample_points: the fields at m query points (the contract is in include/sphx.h).

        points: float32 [m, 2], either a numpy array (host path) or a torch tensor on the context's device (device path).
        fields: any of "density", "fraction", "velocity", "count".  Returns {field: array}: shape [m] ([m, 2] for velocity; count
        uint32 — int32 for torch, which has no uint32 arithmetic), numpy for numpy points, torch tensors for torch points.
        The device path synchronises torch's current stream before the call (the points and the freshly allocated outputs are then
        complete), enqueues the query on the context's own stream and waits for that stream before it returns: the tensors it
        returns hold finished results and no stream of the caller has to be ordered against the library's.  Pass large point sets
        spatially coherent (e.g. sorted by cell): the library processes them in the given order."""
        flags = _sample_fields(fields)
        if _is_torch(points):
            import torch

            if points.device.type != "cuda" or points.dtype != torch.float32 or points.dim() != 2 or points.shape[1] != 2:
                raise ValueError("points must be a float32 [m, 2] tensor on the context's device")
            if self.params is not None and points.device.index not in (None, self.params.device):
                raise ValueError("points are on %s, the context on device %d" % (points.device, self.params.device))
            pts = points.contiguous()
            m = pts.shape[0]
            outs = _torch_outputs(flags, (m,), pts.device)
            torch.cuda.current_stream(pts.device).synchronize()
            self._chk(self.L.sphx_sample_points(self.h, C.c_void_p(pts.data_ptr()), m, kernel, _lib.SAMPLE_DEVICE_POINTERS,
                                                C.byref(_out_struct(outs, lambda t: t.data_ptr()))))
            self.synchronize()
            return outs
        pts = np.ascontiguousarray(points, np.float32)
        if pts.ndim != 2 or pts.shape[1] != 2:
            raise ValueError("points must be a float32 [m, 2] array, not shape %s" % (pts.shape,))
        m = len(pts)
        outs = _numpy_outputs(flags, (m,))
        self._chk(self.L.sphx_sample_points(self.h, _p(pts), m, kernel, 0, C.byref(_out_struct(outs, lambda a: a.ctypes.data))))
        return outs

    def sample_grid(self, origin, spacing, shape, kernel=KERNEL_WENDLAND_C2, fields=SAMPLE_FIELDS):
        """sphx_sample_grid: the fields on the lattice origin + (ix * dx, iy * dy) (fp32, unfused), shape = (ny, nx); row 0 lies at
        origin[1] (the bottom).  spacing: (dx, dy) or one number for both.  Returns {field: numpy array} of shape (ny, nx)
        ((ny, nx, 2) for velocity), bit-identical to sample() at the same fp32 points."""
        flags = _sample_fields(fields)
        dx, dy = (spacing, spacing) if np.ndim(spacing) == 0 else spacing
        ny, nx = (int(v) for v in shape)
        if nx < 0 or ny < 0:
            raise ValueError("shape must be (ny, nx) with non-negative sizes")
        outs = _numpy_outputs(flags, (ny, nx))
        self._chk(self.L.sphx_sample_grid(self.h, origin[0], origin[1], dx, dy, nx, ny, kernel, 0,
                                          C.byref(_out_struct(outs, lambda a: a.ctypes.data))))
        return outs

    def contour(self, origin, spacing, shape, iso=0.5, field="fraction", kind=KERNEL_WENDLAND_C2, cap=None, values=False, out=None):
        """sphx_surface_contour: the contour `field == iso` of the lattice sample_grid(origin, spacing, shape) would return, as directed
        segments with the inside (field >= iso) on their left, in the order of include/sphx.h (cell after cell).

        field: "fraction" or "density"; shape = (ny, nx).  Returns dict(segments [n, 2, 2] = (start, end) x (x, y), cell [n] = the cell
        iy * (nx - 1) + ix of each segment, count = the contour's total number of segments, and values [ny, nx] with values=True).
        cap: the most segments to return (n = min(count, cap)); None calls once with a guessed capacity and once more with the exact
        count if that was too small, so n = count.  cap = 0 returns the count alone.
        Device path: out = dict of torch tensors on the context's device — "segments" float32 [cap, 2, 2] (or [cap, 4]) and / or "cell"
        int32 [cap], optionally "values" float32 [ny, nx]; "count" int32 [1] is allocated when missing.  The tensors are written in
        place (nothing behind min(count, cap) is touched) and the dict returned holds views of their first n entries and count as an
        int.  Like sample(), this path synchronises torch's current stream before the call and the context's stream after it."""
        if field not in _lib.CONTOUR_FIELDS:
            raise ValueError("field must be one of %s, not %r" % (sorted(_lib.CONTOUR_FIELDS), field))
        dx, dy = (spacing, spacing) if np.ndim(spacing) == 0 else spacing
        ny, nx = (int(v) for v in shape)
        if nx < 0 or ny < 0:
            raise ValueError("shape must be (ny, nx) with non-negative sizes")
        o = _lib.SphxContourOut()

        def call(cap_, flags):
            self._chk(self.L.sphx_surface_contour(self.h, origin[0], origin[1], dx, dy, nx, ny, kind, _lib.CONTOUR_FIELDS[field], iso, cap_, flags, C.byref(o)))

        if out is not None:
            import torch

            seg, cel, val = out.get("segments"), out.get("cell"), out.get("values")
            some = next((t for t in (seg, cel, val, out.get("count")) if t is not None), None)
            if some is None or any(t is not None and (not _is_torch(t) or t.device.type != "cuda" or not t.is_contiguous()) for t in (seg, cel, val, out.get("count"))):
                raise ValueError("out must hold contiguous torch tensors on the context's device")
            if seg is not None and (seg.dtype != torch.float32 or seg.dim() < 2 or seg.numel() != 4 * seg.shape[0]):
                raise ValueError("out[\"segments\"] must be a float32 [cap, 2, 2] or [cap, 4] tensor")
            if cel is not None and (cel.dtype != torch.int32 or cel.dim() != 1 or (seg is not None and cel.shape[0] != seg.shape[0])):
                raise ValueError("out[\"cell\"] must be an int32 [cap] tensor, as long as out[\"segments\"]")
            if val is not None and (val.dtype != torch.float32 or val.numel() != nx * ny):
                raise ValueError("out[\"values\"] must be a float32 tensor of ny * nx values")
            cnt = out.get("count")
            if cnt is None:
                cnt = torch.zeros(1, dtype=torch.int32, device=some.device)
            elif cnt.dtype != torch.int32 or cnt.numel() != 1:
                raise ValueError("out[\"count\"] must be an int32 [1] tensor")
            have = seg.shape[0] if seg is not None else (cel.shape[0] if cel is not None else 0)
            cap_ = have if cap is None else min(int(cap), have)
            o.segments = (seg.data_ptr() or 1) if seg is not None and cap_ else None
            o.cell = (cel.data_ptr() or 1) if cel is not None and cap_ else None
            o.values = (val.data_ptr() or 1) if val is not None else None
            o.count = cnt.data_ptr()
            torch.cuda.current_stream(some.device).synchronize()
            call(cap_, _lib.CONTOUR_DEVICE_POINTERS)
            self.synchronize()
            count = int(cnt.item())
            n = min(count, cap_)
            res = dict(count=count)
            if seg is not None:
                res["segments"] = seg.view(-1, 2, 2)[:n]
            if cel is not None:
                res["cell"] = cel[:n]
            if val is not None:
                res["values"] = val.view(ny, nx)
            return res
        cnt = np.zeros(1, np.uint32)
        o.count = cnt.ctypes.data
        val = np.zeros((ny, nx), np.float32) if values else None
        cap_ = max(1024, 8 * (nx + ny)) if cap is None else int(cap)
        while True:
            seg, cel = np.zeros((cap_, 2, 2), np.float32), np.zeros(cap_, np.uint32)
            o.segments, o.cell = (seg.ctypes.data, cel.ctypes.data) if cap_ else (None, None)
            o.values = (val.ctypes.data or 1) if values else None
            call(cap_, 0)
            count = int(cnt[0])
            if cap is not None or count <= cap_:
                break
            cap_ = count
        n = min(count, cap_)
        res = dict(segments=seg[:n], cell=cel[:n], count=count)
        if values:
            res["values"] = val
        return res

    def query(self, points, radius=None, boundary=False, lists=True, nearest=True, cap=None, out=None):
        """sphx_query_radius: the particles within `radius` of m query points, by the box rule of include/sphx.h ("neighbour queries").

        points: float32 [m, 2], a numpy array (host path) or a torch tensor on the context's device (device path).  radius: None = the
        smoothing length h (the largest allowed).  boundary=True answers over the boundary particles (the order of
        download_boundary()) instead of the fluid (the order of download()).
        Returns dict(offsets uint64 [m + 1] (CSR), count = the total number of entries; with lists: index, id uint32 [n] and dist_sq
        float32 [n]; with nearest: nearest uint32 [m] (QUERY_NONE where nothing is accepted) and nearest_dist_sq float32 [m] (+inf
        there)).  cap: the most entries to return (n = min(count, cap)); None makes a count-only call first and sizes the arrays
        exactly, so n = count.
        Device path: the results are torch tensors (int64 offsets, int32 index / id / nearest — torch has no unsigned arithmetic).
        out = dict of contiguous tensors on the context's device to write in place: "offsets" int64 [m + 1], "index" / "id" int32
        [cap], "dist_sq" float32 [cap], "nearest" int32 [m], "nearest_dist_sq" float32 [m], "count" int64 [1]; what is missing is
        allocated according to lists / nearest / cap ("count" always).  Nothing behind min(count, cap) is touched; the dict
        returned holds views of the first n entries and count as an int.  Like sample(), this path synchronises torch's current
        stream before the call and the context's stream after it."""
        if radius is None and self.params is None:
            raise ValueError("radius=None needs the params the context was created with (a borrowed view has none): pass the radius")
        r = float(np.float32(self.params.smoothing_length if radius is None else radius))
        base = _lib.QUERY_BOUNDARY if boundary else 0
        o = _lib.SphxQueryOut()
        if _is_torch(points) or out is not None:
            import torch

            if not _is_torch(points) or points.device.type != "cuda" or points.dtype != torch.float32 or points.dim() != 2 or points.shape[1] != 2:
                raise ValueError("points must be a float32 [m, 2] tensor on the context's device")
            pts = points.contiguous()
            m = pts.shape[0]
            dev = pts.device
            given = dict(out or {})
            want = dict(offsets=(torch.int64, m + 1), index=(torch.int32, None), id=(torch.int32, None), dist_sq=(torch.float32, None),
                        nearest=(torch.int32, m), nearest_dist_sq=(torch.float32, m), count=(torch.int64, 1))
            for k, t in given.items():
                if k not in want:
                    raise ValueError("out has no field %r" % (k,))
                if not _is_torch(t) or t.device.type != "cuda" or not t.is_contiguous() or t.dtype != want[k][0] or t.dim() != 1:
                    raise ValueError("out[%r] must be a contiguous 1-d %s tensor on the context's device" % (k, want[k][0]))
                if want[k][1] is not None and t.numel() != want[k][1]:
                    raise ValueError("out[%r] must hold %d elements" % (k, want[k][1]))
            t_cnt = given.get("count")
            if t_cnt is None:
                t_cnt = torch.zeros(1, dtype=torch.int64, device=dev)
            t_off = given.get("offsets")
            if t_off is None:
                t_off = torch.empty(m + 1, dtype=torch.int64, device=dev)
            t_near, t_nd2 = given.get("nearest"), given.get("nearest_dist_sq")
            if nearest and out is None:
                t_near = torch.empty(m, dtype=torch.int32, device=dev)
                t_nd2 = torch.empty(m, dtype=torch.float32, device=dev)
            ent = {k: given.get(k) for k in ("index", "id", "dist_sq")}
            have = [t.numel() for t in ent.values() if t is not None]
            if len(set(have)) > 1:
                raise ValueError("out[\"index\"], out[\"id\"] and out[\"dist_sq\"] must be equally long")

            def call(cap_, with_lists):
                o.offsets, o.count = t_off.data_ptr(), t_cnt.data_ptr()
                o.nearest = (t_near.data_ptr() or 1) if t_near is not None else None
                o.nearest_dist_sq = (t_nd2.data_ptr() or 1) if t_nd2 is not None else None
                for k, t in ent.items():
                    setattr(o, k, (t.data_ptr() or 1) if with_lists and t is not None and cap_ else None)
                torch.cuda.current_stream(dev).synchronize()
                self._chk(self.L.sphx_query_radius(self.h, C.c_void_p(pts.data_ptr()), m, r, cap_, base | _lib.QUERY_DEVICE_POINTERS, C.byref(o)))
                self.synchronize()
                return int(t_cnt.item())

            if have:
                cap_ = have[0] if cap is None else min(int(cap), have[0])
                count = call(cap_, True)
            elif lists and out is None:
                cap_ = call(0, False) if cap is None else int(cap)
                ent = dict(index=torch.empty(cap_, dtype=torch.int32, device=dev), id=torch.empty(cap_, dtype=torch.int32, device=dev),
                           dist_sq=torch.empty(cap_, dtype=torch.float32, device=dev))
                count = call(cap_, True) if cap_ else (call(0, False) if cap is not None else cap_)
            else:
                cap_, count = 0, call(0, False)
            n = min(count, cap_)
            res = dict(offsets=t_off, count=count)
            res.update({k: t[:n] for k, t in ent.items() if t is not None})
            if t_near is not None:
                res["nearest"] = t_near
            if t_nd2 is not None:
                res["nearest_dist_sq"] = t_nd2
            return res
        pts = np.ascontiguousarray(points, np.float32)
        if pts.ndim != 2 or pts.shape[1] != 2:
            raise ValueError("points must be a float32 [m, 2] array, not shape %s" % (pts.shape,))
        m = len(pts)
        cnt = np.zeros(1, np.uint64)
        off = np.zeros(m + 1, np.uint64)
        near = np.full(m, _lib.QUERY_NONE, np.uint32) if nearest else None
        nd2 = np.full(m, np.inf, np.float32) if nearest else None
        o.offsets, o.count = off.ctypes.data, cnt.ctypes.data
        o.nearest, o.nearest_dist_sq = ((near.ctypes.data or 1), (nd2.ctypes.data or 1)) if nearest else (None, None)
        res = dict(offsets=off)
        if nearest:
            res.update(nearest=near, nearest_dist_sq=nd2)
        cap_ = int(cap) if cap is not None else 0
        if cap is None or not lists:
            self._chk(self.L.sphx_query_radius(self.h, _p(pts), m, r, 0, base, C.byref(o)))  # count only: one walk
            cap_ = int(cnt[0]) if cap is None else cap_
        if lists:
            idx, ids, d2 = np.zeros(cap_, np.uint32), np.zeros(cap_, np.uint32), np.zeros(cap_, np.float32)
            if cap is not None or cap_:
                o.index, o.id, o.dist_sq = ((idx.ctypes.data, ids.ctypes.data, d2.ctypes.data) if cap_ else (None, None, None))
                self._chk(self.L.sphx_query_radius(self.h, _p(pts), m, r, cap_, base, C.byref(o)))
            n = min(int(cnt[0]), cap_)
            res.update(index=idx[:n], id=ids[:n], dist_sq=d2[:n])
        res["count"] = int(cnt[0])
        return res

    def select(self, rects, outside=False, cap=None, out=None):
        """sphx_select: the particles sphx_remove(rects, outside) would remove, in ascending device index — and nothing is removed.

        rects: as remove().  Returns dict(index uint32 [n] (the order of download()), id uint32 [n] (particle_id), count = the number
        selected).  cap: the most to return (n = min(count, cap)); None makes a count-only call first, so n = count.
        Device path: out = dict of contiguous int32 torch tensors on the context's device, "index" and / or "id" [cap] and optionally
        "count" [1]; they are written in place (nothing behind min(count, cap) is touched) and views of the first n come back."""
        arr, k = _rect_array(rects)
        base = _lib.SELECT_OUTSIDE if outside else 0
        o = _lib.SphxSelectOut()
        if out is not None:
            import torch

            idx, ids, t_cnt = out.get("index"), out.get("id"), out.get("count")
            some = next((t for t in (idx, ids, t_cnt) if t is not None), None)
            if some is None or any(t is not None and (not _is_torch(t) or t.device.type != "cuda" or not t.is_contiguous() or t.dtype != torch.int32
                                                      or t.dim() != 1) for t in (idx, ids, t_cnt)):
                raise ValueError("out must hold contiguous 1-d int32 torch tensors on the context's device")
            if idx is not None and ids is not None and idx.numel() != ids.numel():
                raise ValueError("out[\"index\"] and out[\"id\"] must be equally long")
            if t_cnt is None:
                t_cnt = torch.zeros(1, dtype=torch.int32, device=some.device)
            elif t_cnt.numel() != 1:
                raise ValueError("out[\"count\"] must be an int32 [1] tensor")
            have = idx.numel() if idx is not None else (ids.numel() if ids is not None else 0)
            cap_ = have if cap is None else min(int(cap), have)
            o.index = (idx.data_ptr() or 1) if idx is not None and cap_ else None
            o.id = (ids.data_ptr() or 1) if ids is not None and cap_ else None
            o.count = t_cnt.data_ptr()
            torch.cuda.current_stream(some.device).synchronize()
            self._chk(self.L.sphx_select(self.h, arr, k, base | _lib.SELECT_DEVICE_POINTERS, cap_, C.byref(o)))
            self.synchronize()
            count = int(t_cnt.item())
            n = min(count, cap_)
            res = dict(count=count)
            if idx is not None:
                res["index"] = idx[:n]
            if ids is not None:
                res["id"] = ids[:n]
            return res
        cnt = np.zeros(1, np.uint32)
        o.count = cnt.ctypes.data
        if cap is None:
            self._chk(self.L.sphx_select(self.h, arr, k, base, 0, C.byref(o)))
            cap_ = int(cnt[0])
        else:
            cap_ = int(cap)
        idx, ids = np.zeros(cap_, np.uint32), np.zeros(cap_, np.uint32)
        if cap is not None or cap_:
            o.index, o.id = (idx.ctypes.data, ids.ctypes.data) if cap_ else (None, None)
            self._chk(self.L.sphx_select(self.h, arr, k, base, cap_, C.byref(o)))
        n = min(int(cnt[0]), cap_)
        return dict(index=idx[:n], id=ids[:n], count=int(cnt[0]))

    def render(self, view=None, *, out=None, owner=False, rgba=True, **view_fields):
        """sphx_render: the particles drawn as discs (the contract is in include/sphx.h).

        view: a SphxRenderView (render_fit); None = render_fit(width, height, world_rect) with width = 1920, height = 1080 and
        world_rect = SCENE_RECT unless given among view_fields.  Other view_fields override single fields of (a copy of) the view.
        Host path (out None): returns the image as a uint8 (H, W, 4) numpy array; with owner=True the pair (image, uint32 (H, W) owners:
        a device index, _lib.RENDER_BOUNDARY or _lib.RENDER_NONE); with rgba=False the owners alone.
        Device path: out = a torch uint8 tensor of shape (H, W, 4) on the context's device (or None with rgba=False) — the image is
        written into it; owner=True allocates an int32 (H, W) tensor, owner=<such a tensor> uses it (torch has no uint32 arithmetic: the
        two codes read -1 and -2).
        Like sample(), the device path synchronises torch's current stream before the call and the context's stream after it."""
        if view is None:
            width, height = view_fields.pop("width", 1920), view_fields.pop("height", 1080)
            view = render_fit(width, height, view_fields.pop("world_rect", SCENE_RECT))
        else:
            view = _copy_view(view)
        _set_view_fields(view, view_fields)
        owner_tensor = owner if _is_torch(owner) else None
        owner = owner_tensor is not None or bool(owner)
        if not rgba and not owner:
            raise ValueError("nothing to render: rgba and owner are both off")
        h, w = view.height, view.width
        o = _lib.SphxRenderOut()
        if out is not None or owner_tensor is not None:
            import torch

            dev = out.device if out is not None else owner_tensor.device
            if out is not None and (not _is_torch(out) or out.device.type != "cuda" or out.dtype != torch.uint8 or tuple(out.shape) != (h, w, 4)
                                    or not out.is_contiguous()):
                raise ValueError("out must be a contiguous uint8 (%d, %d, 4) tensor on the context's device" % (h, w))
            if not rgba and out is not None:
                raise ValueError("out given with rgba=False")
            own = None
            if owner:
                own = owner_tensor if owner_tensor is not None else torch.empty((h, w), dtype=torch.int32, device=dev)
                if own.dtype != torch.int32 or tuple(own.shape) != (h, w) or not own.is_contiguous() or own.device != dev:
                    raise ValueError("owner must be a contiguous int32 (%d, %d) tensor on the device of out" % (h, w))
            o.rgba = (out.data_ptr() or 1) if out is not None else None
            o.owner = (own.data_ptr() or 1) if own is not None else None
            torch.cuda.current_stream(dev).synchronize()
            self._chk(self.L.sphx_render(self.h, C.byref(view), _lib.RENDER_DEVICE_POINTERS, C.byref(o)))
            self.synchronize()
            return own if out is None else ((out, own) if own is not None else out)
        img = np.zeros((h, w, 4), np.uint8) if rgba else None
        own = np.zeros((h, w), np.uint32) if owner else None
        o.rgba = (img.ctypes.data or 1) if rgba else None
        o.owner = (own.ctypes.data or 1) if owner else None
        self._chk(self.L.sphx_render(self.h, C.byref(view), 0, C.byref(o)))
        return own if not rgba else ((img, own) if owner else img)

    def state_size(self):
        """sphx_state_size: bytes of the blob save_state() would write now."""
        n = C.c_uint64()
        self._chk(self.L.sphx_state_size(self.h, C.byref(n)))
        return n.value

    def save_state(self, device=False):
        """sphx_state_save: everything a later step can read, as one blob (the contract is in include/sphx.h).

        -> a numpy uint8 array; with device=True a torch uint8 tensor on the context's device (the sections are copied device to
        device).  Like sample() and render(), the device path synchronises torch's current stream before the call; the library waits
        for its own stream before it returns, so the tensor is complete."""
        size = self.state_size()
        done = C.c_uint64()
        if device:
            import torch

            dev = torch.device("cuda", self.params.device if self.params is not None else torch.cuda.current_device())
            blob = torch.empty(size, dtype=torch.uint8, device=dev)
            torch.cuda.current_stream(dev).synchronize()
            self._chk(self.L.sphx_state_save(self.h, C.c_void_p(blob.data_ptr()), size, _lib.STATE_DEVICE_BUFFER, C.byref(done)))
        else:
            blob = np.empty(size, np.uint8)
            self._chk(self.L.sphx_state_save(self.h, _p(blob), size, 0, C.byref(done)))
        assert done.value == size
        return blob

    def load_state(self, blob):
        """sphx_state_load: blob = bytes / bytearray / memoryview, a numpy uint8 array, or a torch uint8 tensor (a cuda tensor on the
        context's device takes the device path: torch's current stream is synchronised first, and the library is done with the tensor
        when the call returns)."""
        if _is_torch(blob):
            import torch

            if blob.dtype != torch.uint8 or blob.dim() != 1:
                raise ValueError("blob must be a 1-D uint8 tensor")
            if blob.device.type == "cuda":
                if self.params is not None and blob.device.index not in (None, self.params.device):
                    raise ValueError("blob is on %s, the context on device %d" % (blob.device, self.params.device))
                t = blob.contiguous()
                torch.cuda.current_stream(t.device).synchronize()
                self._chk(self.L.sphx_state_load(self.h, C.c_void_p(t.data_ptr() or 1), t.numel(), _lib.STATE_DEVICE_BUFFER))
                return
            blob = blob.numpy()
        a = np.frombuffer(blob, np.uint8) if isinstance(blob, (bytes, bytearray, memoryview)) else np.ascontiguousarray(blob, np.uint8).reshape(-1)
        self._chk(self.L.sphx_state_load(self.h, C.c_void_p(a.ctypes.data or 1), a.size, 0))

    def state_digest(self):
        """sphx_state_digest: {section name: 64-bit digest} of the live state (_lib.STATE_SECTIONS); 72 bytes come back from the device.
        An integrity check and a fingerprint for comparing two contexts or runs, not a cryptographic hash."""
        out = (C.c_uint64 * len(_lib.STATE_SECTIONS))()
        self._chk(self.L.sphx_state_digest(self.h, out))
        return {name: int(out[k]) for k, name in enumerate(_lib.STATE_SECTIONS)}

    def save_state_file(self, path):
        self._chk(self.L.sphx_state_save_file(self.h, str(path).encode()))

    def load_state_file(self, path):
        self._chk(self.L.sphx_state_load_file(self.h, str(path).encode()))

    def profile_enable(self, on=True):
        self._chk(self.L.sphx_profile_enable(self.h, int(on)))

    def profile_filter(self, label=None, every=1):
        """Time only every `every`-th launch with this label (None = all launches)."""
        self._chk(self.L.sphx_profile_filter(self.h, label.encode() if label else None, every))

    def profile_reset(self):
        self._chk(self.L.sphx_profile_reset(self.h))

    def profile_event_overhead(self):
        """Mean elapsed ms of an EMPTY hipEvent bracket on the context's stream (what the bracket adds to a timed launch)."""
        v = C.c_double()
        self._chk(self.L.sphx_profile_event_overhead(self.h, C.byref(v)))
        return v.value

    def profile_get(self):
        n = C.c_uint32(0)
        self._chk(self.L.sphx_profile_get(self.h, None, C.byref(n)))
        arr = (SphxKernelTime * max(1, n.value))()
        self._chk(self.L.sphx_profile_get(self.h, arr, C.byref(n)))
        return {arr[i].name.decode(): dict(launches=arr[i].launches, total_ms=arr[i].total_ms, bytes=arr[i].algorithmic_bytes)
                for i in range(n.value)}


class FluidParticleWorld:
    """Host-side world (fluidparticleworld.rs:92-195): scene helpers + the host copies of the particle arrays."""

    def __init__(self, smoothing_factor=2.0, particle_density=10000.0, fluid_density=100.0):
        self.L = _lib.lib()
        self.h = self.L.sphx_world_create(smoothing_factor, particle_density, fluid_density)
        if not self.h:
            raise ValueError("particle_density must be positive")
        self.args = (smoothing_factor, particle_density, fluid_density)

    def close(self):
        if getattr(self, "h", None):
            self.L.sphx_world_destroy(self.h)
            self.h = None

    __del__ = close

    def properties(self):
        out = np.zeros(4, np.float32)
        self.L.sphx_world_properties(self.h, _p(out))
        return dict(smoothing_length=out[0], particle_mass=out[1], particle_radius=out[2], fluid_density=out[3])

    def remove_all_fluid_particles(self):
        self.L.sphx_world_remove_all_fluid_particles(self.h)

    def remove_all_boundary_particles(self):
        self.L.sphx_world_remove_all_boundary_particles(self.h)

    def add_fluid_rect(self, x, y, w, h, jitter_amount):
        self.L.sphx_world_add_fluid_rect(self.h, x, y, w, h, jitter_amount)

    def add_boundary_thick_line(self, start, end, thickness_in_particles):
        self.L.sphx_world_add_boundary_thick_line(self.h, start[0], start[1], end[0], end[1], thickness_in_particles)

    def add_boundary_line(self, start, end):
        self.L.sphx_world_add_boundary_line(self.h, start[0], start[1], end[0], end[1])

    def reset_fluid(self, scale=1.0):
        """main.rs:177-196 dam-break scene, every coordinate multiplied by `scale`."""
        self.L.sphx_world_reset_fluid(self.h, scale)

    def set_particles(self, pos, vel=None):
        pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 2)
        if vel is not None:
            vel = np.ascontiguousarray(vel, np.float32).reshape(-1, 2)
        self.L.sphx_world_set_particles(self.h, _p(pos), _p(vel), len(pos))

    def set_boundary(self, xy):
        xy = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
        self.L.sphx_world_set_boundary(self.h, _p(xy), len(xy))

    @property
    def num_dynamic_particles(self):
        return self.L.sphx_world_num_dynamic_particles(self.h)

    @property
    def num_boundary_particles(self):
        return self.L.sphx_world_num_boundary_particles(self.h)

    def _view(self, ptr, shape, dtype):
        n = int(np.prod(shape))
        if not ptr or n == 0:
            return np.zeros(shape, dtype)
        ct = {np.float32: C.c_float, np.uint32: C.c_uint32}[dtype]
        return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(ct)), shape=(n,)).reshape(shape).copy()

    @property
    def positions(self):
        return self._view(self.L.sphx_world_positions(self.h), (self.num_dynamic_particles, 2), np.float32)

    @property
    def velocities(self):
        return self._view(self.L.sphx_world_velocities(self.h), (self.num_dynamic_particles, 2), np.float32)

    @property
    def densities(self):
        return self._view(self.L.sphx_world_densities(self.h), (self.num_dynamic_particles,), np.float32)

    @property
    def boundary_particles(self):
        return self._view(self.L.sphx_world_boundary(self.h), (self.num_boundary_particles, 2), np.float32)

    @property
    def particle_ids(self):
        return self._view(self.L.sphx_world_particle_ids(self.h), (self.num_dynamic_particles,), np.uint32)


class TimeManager:
    """timemanager.rs, simulation clock only.  Defaults are the reference app's DFSPH values (main.rs:115-129)."""

    def __init__(self, timestep_max_ns=None, timestep_min_ns=None, cfl_factor=1.5, fixed_ns=None):
        self.L = _lib.lib()
        if fixed_ns is not None:
            self.h = self.L.sphx_timer_create_fixed(fixed_ns)
        else:
            if timestep_max_ns is None:
                timestep_max_ns = duration_from_secs_f32(np.float32(1.0) / np.float32(120.0) / np.float32(3.0))
            if timestep_min_ns is None:
                timestep_min_ns = duration_from_secs_f32(np.float32(1.0) / np.float32(60.0) / np.float32(400.0))
            self.h = self.L.sphx_timer_create_adaptive(timestep_max_ns, timestep_min_ns, cfl_factor)
        self.timestep_max_ns, self.timestep_min_ns, self.cfl_factor = timestep_max_ns, timestep_min_ns, cfl_factor

    def close(self):
        if getattr(self, "h", None):
            self.L.sphx_timer_destroy(self.h)
            self.h = None

    __del__ = close

    def restart(self):
        self.L.sphx_timer_restart(self.h)

    def simulation_step_ns(self):
        return self.L.sphx_timer_simulation_step_ns(self.h)

    def simulation_step(self):
        return duration_as_secs_f32(self.simulation_step_ns())

    def update_simulation_step(self, particle_diameter, max_velocity):
        return self.L.sphx_timer_update_simulation_step(self.h, particle_diameter, max_velocity)

    def set_target_frame(self, target_ns):
        """AdaptiveTimeStepTarget::TargetFrameLength (timemanager.rs:24-36); 0 = None."""
        self.L.sphx_timer_set_target_frame(self.h, target_ns)

    def on_step_started(self):
        """The clock part of simulation_frame_loop (timemanager.rs:244-247): total simulated time advances by the current step."""
        self.L.sphx_timer_on_step_started(self.h)

    def law(self, particle_diameter):
        """sphx_timer_law for SphxContext.step_begin: this timer's config and current step."""
        out = _lib.SphxTimerLaw()
        rc = self.L.sphx_timer_law_of(self.h, particle_diameter, C.byref(out))
        if rc:
            raise SphxError(rc, "sphx_timer_law_of")
        return out

    def get_state(self):
        """sphx_timer_get_state: everything the timer holds, as a _lib.SphxTimerState."""
        st = _lib.SphxTimerState()
        rc = self.L.sphx_timer_get_state(self.h, C.byref(st))
        if rc:
            raise SphxError(rc, "sphx_timer_get_state")
        return st

    def set_state(self, state):
        """sphx_timer_set_state: continue exactly as the timer that get_state() was taken from."""
        rc = self.L.sphx_timer_set_state(self.h, C.byref(state))
        if rc:
            raise SphxError(rc, "sphx_timer_set_state: not a state a TimeManager can hold")
        self.timestep_max_ns, self.timestep_min_ns, self.cfl_factor = state.timestep_max_ns, state.timestep_min_ns, state.cfl_factor

    @property
    def total_simulated_ns(self):
        return self.L.sphx_timer_total_simulated_ns(self.h)

    @property
    def num_steps(self):
        return self.L.sphx_timer_num_steps(self.h)


class DFSPHSolver:
    """Box<dyn Solver> holding the HIP-backed DFSPHSolver (solver/mod.rs:12-18, dfsph.rs:405-526)."""

    _create = "sphx_solver_create_dfsph"

    def __init__(self, world, params=None):
        self.L = _lib.lib()
        h = C.c_void_p()
        rc = getattr(self.L, self._create)(world.h, C.byref(params) if params is not None else None, C.byref(h))
        if rc:
            raise SphxError(rc, self.L.sphx_last_error(None).decode())
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.L.sphx_solver_destroy(self.h)
            self.h = None

    __del__ = close

    def clear_cached_data(self):
        self.L.sphx_solver_clear_cached_data(self.h)

    def simulation_step(self, world, time_manager, sync_world=True):
        st = SphxStepStats()
        rc = self.L.sphx_solver_simulation_step(self.h, world.h, time_manager.h, int(sync_world), C.byref(st))
        if rc:
            raise SphxError(rc, self.L.sphx_solver_last_error(self.h).decode())
        return st.as_dict()

    def simulation_steps(self, world, time_manager, k, sync_world=True):
        """k consecutive simulation_step calls inside the library (the frame loop of main.rs:348-350); returns the k stats dicts."""
        st = (SphxStepStats * k)()
        done = C.c_uint32()
        rc = self.L.sphx_solver_simulation_steps(self.h, world.h, time_manager.h, int(sync_world), k, st, C.byref(done))
        if rc:
            raise SphxError(rc, f"step {done.value} of {k}: " + self.L.sphx_solver_last_error(self.h).decode())
        return [x.as_dict() for x in st]

    def sync_world(self, world):
        rc = self.L.sphx_solver_sync_world(self.h, world.h)
        if rc:
            raise SphxError(rc, self.L.sphx_solver_last_error(self.h).decode())

    def append(self, world, pos, vel=None, sync_world=True):
        """sphx_solver_append: SphxContext.append on the solver's device state; the world follows (sync_world=False: its arrays are
        only marked as behind the device).  No re-upload follows, ids survive. -> the id of the first new particle."""
        pos, vel = _append_arrays(pos, vel)
        first = C.c_uint32()
        rc = self.L.sphx_solver_append(self.h, world.h, _p(pos), _p(vel), len(pos), int(sync_world), C.byref(first))
        if rc:
            raise SphxError(rc, self.L.sphx_solver_last_error(self.h).decode())
        return first.value

    def remove(self, world, rects, outside=False, sync_world=True):
        """sphx_solver_remove: SphxContext.remove on the solver's device state; the world follows as in append(). -> the number removed."""
        arr, k = _rect_array(rects)
        removed = C.c_uint32()
        rc = self.L.sphx_solver_remove(self.h, world.h, arr, k, _lib.REMOVE_OUTSIDE if outside else 0, int(sync_world), C.byref(removed))
        if rc:
            raise SphxError(rc, self.L.sphx_solver_last_error(self.h).decode())
        return removed.value

    def save(self, world, time_manager, path):
        """sphx_solver_save: one file holding the context's blob and the timer's state."""
        rc = self.L.sphx_solver_save(self.h, world.h, time_manager.h, str(path).encode())
        if rc:
            raise SphxError(rc, self.L.sphx_solver_last_error(self.h).decode())

    def load(self, world, time_manager, path, sync_world=False):
        """sphx_solver_load: continue the run of the file; the timer gets the saved state, the world the saved boundary and the device's
        particle count (sync_world=True also downloads its arrays)."""
        rc = self.L.sphx_solver_load(self.h, world.h, time_manager.h, str(path).encode())
        if rc:
            raise SphxError(rc, self.L.sphx_solver_last_error(self.h).decode())
        if sync_world:
            self.sync_world(world)

    def context(self):
        """Borrowed SphxContext view (for inspection: neighbours, cells, solver state, profiling — and for following particles: the
        tracked set and the recorder live on the context, and the recorder fires behind every step of simulation_steps(k)):

            ctx = solver.context()
            ctx.track([0, 17, 4049])
            ctx.track_record(max_frames=100)
            solver.simulation_steps(world, timer, 100, sync_world=False)
            paths = ctx.track_frames()  # [100, 3, 4] = x, y, vx, vy after each step
        """
        ctx = SphxContext.__new__(SphxContext)
        ctx.L = self.L
        ctx.params = None
        ctx._owned = False
        ctx.h = C.c_void_p(self.L.sphx_solver_ctx(self.h))
        return ctx


class DFSPHMultiSolver(DFSPHSolver):
    """The same Box<dyn Solver> over several GPUs (sph::HipDfsphMultiSolver): simulation_step / clear_cached_data / sync_world as before,
    the tiles, the halo exchange and the reductions live inside libsphx (sphx_multi)."""

    def __init__(self, world, devices, params=None, options=None):
        self.L = _lib.lib()
        h = C.c_void_p()
        devs = (C.c_int * len(devices))(*devices)
        rc = self.L.sphx_solver_create_dfsph_multi(world.h, C.byref(params) if params is not None else None, devs, len(devices),
                                                   C.byref(options) if options is not None else None, C.byref(h))
        if rc:
            raise SphxError(rc, self.L.sphx_multi_last_error(None).decode())
        self.h = h

    def multi(self):
        """Borrowed MultiSolver view of the tiles behind this solver (statistics, info, tile contexts); the solver keeps owning them."""
        from .multi import MultiSolver

        m = MultiSolver.__new__(MultiSolver)
        m.L, m.params, m._borrowed = self.L, None, True
        m.h = C.c_void_p(self.L.sphx_solver_multi(self.h))
        return m

    # fluid statistics of the tiled run (MultiSolver.stats and its recorder; the recorder fires behind every step of simulation_steps(k))
    def stats(self, rects=(), per_tile=False):
        return self.multi().stats(rects, per_tile)

    def stats_record(self, rects, max_frames, every=1):
        self.multi().stats_record(rects, max_frames, every)

    def stats_status(self):
        return self.multi().stats_status()

    def stats_frames(self, first=0, count=None):
        return self.multi().stats_frames(first, count)

    # sampling the fields of the tiled run (MultiSolver.sample / sample_grid: answered by the tiles, no download; gauge_elevation takes
    # this solver or its multi() as it takes a SphxContext)
    def sample(self, points, kernel=KERNEL_WENDLAND_C2, fields=SAMPLE_FIELDS, tiles=False):
        return self.multi().sample(points, kernel, fields, tiles)

    def sample_grid(self, origin, spacing, shape, kernel=KERNEL_WENDLAND_C2, fields=SAMPLE_FIELDS, tiles=False):
        return self.multi().sample_grid(origin, spacing, shape, kernel, fields, tiles)

    # gauges and probes of the tiled run (MultiSolver.gauges and its recorder; the recorder fires behind every step of simulation_steps(k))
    def gauges(self, gauges, iso=0.5, field="fraction", kernel=KERNEL_WENDLAND_C2, values=False, tiles=False):
        return self.multi().gauges(gauges, iso, field, kernel, values, tiles)

    def probe_record(self, points=None, gauges=None, max_frames=0, every=1, iso=0.5, field="fraction", kernel=KERNEL_WENDLAND_C2):
        self.multi().probe_record(points, gauges, max_frames, every, iso, field, kernel)

    def probe_status(self):
        return self.multi().probe_status()

    def probe_frames(self, first=0, count=None, tiles=False):
        return self.multi().probe_frames(first, count, tiles)

    # the free surface of the tiled run (MultiSolver.contour: cut by the tiles, merged on the host in cell order)
    def contour(self, origin, spacing, shape, iso=0.5, field="fraction", kind=KERNEL_WENDLAND_C2, cap=None, tiles=False):
        return self.multi().contour(origin, spacing, shape, iso, field, kind, cap, tiles)

    # per-particle flow fields of the tiled run (MultiSolver.fields: computed by the tiles over their own arrays, no download)
    def fields(self, fields=FIELD_NAMES, by_id=False):
        return self.multi().fields(fields, by_id)

    # neighbour queries of the tiled run (MultiSolver.query / select: answered by the tiles over their own arrays, nothing is exchanged;
    # the borrowed view has no params, so the radius is required)
    def query(self, points, radius=None, boundary=False, lists=True, nearest=True, cap=None, tiles=False):
        return self.multi().query(points, radius, boundary, lists, nearest, cap, tiles)

    def select(self, rects, outside=False, cap=None, by_id=False):
        return self.multi().select(rects, outside, cap, by_id)

    # following particles by id (MultiSolver.track and friends; the recorder fires behind every step of simulation_steps(k))
    def track(self, ids):
        self.multi().track(ids)

    def track_fetch(self, fields=None):
        return self.multi().track_fetch(fields)

    def track_record(self, max_frames, every=1):
        self.multi().track_record(max_frames, every)

    def track_status(self):
        return self.multi().track_status()

    def track_frames(self, first=0, count=None, tiles=False):
        return self.multi().track_frames(first, count, tiles)

    def download_by_id(self, first=0, count=None, fields=None):
        return self.multi().download_by_id(first, count, fields)

    # the picture of the tiled run (MultiSolver.render / render_layer: drawn by the tiles, merged on the host; owners are particle ids)
    def render(self, view=None, *, owner=False, rgba=True, **view_fields):
        return self.multi().render(view, owner=owner, rgba=rgba, **view_fields)

    def render_layer(self, view=None, **view_fields):
        return self.multi().render_layer(view, **view_fields)

    # the tiled run put down and picked up (save / load of the base class keep refusing this solver)
    def checkpoint(self, world, time_manager, path):
        """sphx_solver_multi_checkpoint: one file holding the part(s) of MultiSolver.save_state() and the timer's state."""
        rc = self.L.sphx_solver_multi_checkpoint(self.h, world.h, time_manager.h, str(path).encode())
        if rc:
            raise SphxError(rc, self.L.sphx_solver_last_error(self.h).decode())

    def restore(self, world, time_manager, path, sync_world=False):
        """sphx_solver_multi_restore: continue the run of the file; the timer gets the saved state, the world the saved boundary and the
        run's particle count (sync_world=True also downloads its arrays)."""
        rc = self.L.sphx_solver_multi_restore(self.h, world.h, time_manager.h, str(path).encode())
        if rc:
            raise SphxError(rc, self.L.sphx_solver_last_error(self.h).decode())
        if sync_world:
            self.sync_world(world)


class WCSPHSolver(DFSPHSolver):
    """Box<dyn Solver> holding the HIP-backed WCSPHSolver (solver/wscsph.rs); the app pairs it with cfl_factor 0.2 (main.rs:116-119)."""

    _create = "sphx_solver_create_wcsph"
