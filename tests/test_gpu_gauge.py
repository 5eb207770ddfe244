"""Gauges and probes on the device (sphx_gauge_levels, sphx_probe_*): the values are sphx_sample_points' bits, the records the rule's
(sphx_gauge_reduce and the numpy restatement, tests/gauge_reference.py), at the shapes at which the two kernels can go wrong; the
crossing is the contour's; device pointers, canaries, determinism, the state rules and argument errors of include/sphx.h; the recorder
against one-shot calls of a twin run, its bookkeeping and lifetime; no side effects on a run; the harness's --gauge-out."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import gauge_reference as gr
import sample_reference as sr
import yasph2d_amd as y
from util import dam_break
from yasph2d_amd import _lib

pytestmark = pytest.mark.gpu

F = np.float32
KINDS = (y.KERNEL_WENDLAND_C2, y.KERNEL_POLY6, y.KERNEL_SPIKY)
DIAM = F(0.01)
HARNESS = os.path.join(os.path.dirname(os.path.abspath(y.__file__)), "sphx_harness")
ISO = {"fraction": 0.5, "density": 60.0}

# The scene (main.rs:177-196): walls around [0, 2] x [0, 2.5], the fluid block [0.1, 0.6] x [0.7, 1.7] on a ramp from (0, 0.6) down to
# (1.75, 0.5), the floor at y = 0 below it.  Vertical rays, horizontal ones (the front along the floor: dy == 0), one along the ramp, a
# downward and two oblique ones; one ray wholly outside the domain (below grid_min = -100) and two with huge coordinates.
RAYS = [[x, 0.0, 0.0, 0.005, 400] for x in (0.05, 0.2, 0.35, 1.0, 1.9)] + \
       [[0.0, 0.02, 0.004, 0.0, 500], [0.3, 2.0, 0.0, -0.006, 350], [0.0, 0.0, 0.0031, 0.0047, 300], [1.9, 1.5, -0.0043, -0.0029, 400],
        [0.02, 0.63, 0.004, -0.004 * 0.1 / 1.75, 490], [0.0, 0.9, 0.004, 0.0, 500],
        [-150.0, -150.0, 0.1, 0.0, 50], [3e38, -3e38, 1e36, 1e36, 40], [1e30, 0.5, -1e28, 0.0, 65]]
POINTS = np.array([[0.05, 0.05], [0.3, 0.4], [0.3, 0.9], [1.0, 0.02], [1.95, 0.1], [0.6, 1.2], [-3.0, 0.5], [np.nan, 0.1]], F)


def dfsph_step(ctx, timer, log=None):
    vmax = ctx.step_begin(timer.simulation_step(), timer.law(DIAM))
    dt = y.duration_as_secs_f32(timer.update_simulation_step(DIAM, vmax))
    st = ctx.step_finish(dt)
    if log is not None:
        log.append((np.float32(vmax), timer.simulation_step_ns(), st, ctx.last_flags()))
    return dt


def wcsph_step(ctx, timer, log=None):
    vmax = ctx.wcsph_step_begin(timer.simulation_step())
    dt = y.duration_as_secs_f32(timer.update_simulation_step(DIAM, vmax))
    st = ctx.wcsph_step_finish(dt)
    if log is not None:
        log.append((np.float32(vmax), timer.simulation_step_ns(), st, ctx.last_flags()))
    return dt


def scene_ctx():
    pos, bnd = dam_break(1.0)
    ctx = y.SphxContext()
    ctx.set_boundary(bnd)
    ctx.upload(pos)
    return ctx


def words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def check_call(ctx, gauges, iso, field="fraction", kind=y.KERNEL_WENDLAND_C2, what=""):
    """one call: the values are ctx.sample's bits at the gauges' fp32 points, the records the rule's over those values"""
    rec, val = ctx.gauges(gauges, iso, field, kind, values=True)
    pts = gr.all_points(gauges)
    assert np.array_equal(words(val), words(ctx.sample(pts, kind, fields=(field,))[field])), "%s: values differ from sample()" % what
    assert gr.same_bytes(rec, y.gauge_reduce(val, gauges, iso)), "%s: records differ from gauge_reduce(values)" % what
    assert gr.same_bytes(rec, gr.reduce32(val, gauges, iso)), "%s: records differ from the restatement" % what
    assert gr.same_bytes(ctx.gauges(gauges, iso, field, kind), rec), "%s: without values" % what
    return rec, val


def check_state(ctx, what, restated=False):
    for kind in KINDS:
        for field in ("fraction", "density"):
            rec, val = check_call(ctx, RAYS, ISO[field], field, kind, "%s kind %d %s" % (what, kind, field))
            assert not val[-155:].any() and (rec["inside"][-3:] == 0).all() and (rec["first"][-3:] == gr.NONE).all()  # outside the domain, huge coordinates: sampling's zeros
            at = 0
            for g in RAYS[:5]:  # a vertical gauge is column 0 of the lattice
                col = ctx.sample_grid((F(g[0]), F(g[1])), (F(7.0), F(g[3])), (g[4], 1), kind, fields=(field,))[field][:, 0]
                assert np.array_equal(words(col), words(val[at:at + g[4]]))
                at += g[4]
    if restated:  # the whole chain in numpy: restated sampling, restated rule
        d = ctx.download()
        st = dict(pos=d["pos"], vel=d["vel"], density=d["density"], boundary=ctx.download_boundary()[0])
        rec, val = ctx.gauges(RAYS, 0.5, values=True)
        rref, vref = gr.levels32(sr.Constants(ctx.params, ctx.constants()), st, RAYS, 0.5)
        assert np.array_equal(words(val), words(vref)) and gr.same_bytes(rec, rref), what
    return ctx.gauges(RAYS, 0.5)


# ---- 1. bit parity ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dam400():
    """the dam break after 400 DFSPH steps (checked on the way after 1 and 50), shared read-only"""
    ctx, timer, done, recs = scene_ctx(), y.TimeManager(), 0, {}
    for k in (1, 50, 400):
        for _ in range(k - done):
            dfsph_step(ctx, timer)
        done = k
        recs[k] = check_state(ctx, "DFSPH step %d" % k, restated=(k == 50))
    return ctx, recs


@pytest.fixture(scope="module")
def dam1():
    """the dam break after one DFSPH step: the block still stands, shared read-only"""
    ctx = scene_ctx()
    dfsph_step(ctx, y.TimeManager())
    return ctx


def test_bit_parity_dfsph_1_50_400(dam400):
    ctx, recs = dam400
    r = recs[1]
    assert (r["inside"][1:3] > 150).all() and (r["inside"][[0, 3, 4]] == 0).all()  # the block stands over x = 0.2 and 0.35, the rest is dry
    assert r["inside"][10] > 100 and 0.55 < r["x"][10] < 0.65 and r["y"][10] == F(0.9)  # a horizontal ray leaves the block near x = 0.6
    assert 0 < r["first"][6] < r["last"][6] < 349  # a downward ray enters and leaves the block
    assert r["inside"][9] == 0 and recs[400]["inside"][9] > 0 and recs[400]["x"][9] > 0.6  # the front runs down the ramp


def test_bit_parity_wcsph_30():
    ctx, timer = scene_ctx(), y.TimeManager(cfl_factor=0.2)
    for _ in range(30):
        wcsph_step(ctx, timer)
    rec = check_state(ctx, "WCSPH step 30")
    assert (rec["inside"][1:3] > 100).all()


# ---- 2. the shapes at which the kernels can go wrong ----------------------------------------------------------------------------------
def test_mixed_lengths_and_gauge_counts(dam400):
    ctx, _ = dam400
    lengths = [1, 2, 63, 64, 65, 255, 256, 257, 1025]
    mixed = [[0.03 + 0.11 * k, 0.004, 0.0, 1.2 / n, n] for k, n in enumerate(lengths)]
    rec, val = check_call(ctx, mixed, 0.5, what="mixed lengths")
    assert len(val) == sum(lengths) and (rec["inside"] > 0).sum() >= 2
    check_call(ctx, mixed[::-1], 0.5, "density", y.KERNEL_POLY6, what="mixed lengths, reversed")
    rng = np.random.default_rng(4)
    for g in (1, 2, 65, _lib.GAUGE_MAX):
        many = [[rng.uniform(0.0, 2.0), rng.uniform(0.0, 0.1), rng.uniform(-0.001, 0.001), 0.03, 37] for _ in range(g)]
        rec, _ = check_call(ctx, many, 0.5, what="%d gauges" % g)
        assert len(rec) == g and (g < 65 or (rec["inside"] > 0).any())
    assert len(ctx.gauges([])) == 0 and len(ctx.gauges(None)) == 0  # n_gauges == 0 succeeds


def test_last_on_the_trip_wavefront_and_workgroup_edges(dam1):
    """Columns whose y0 is chosen from a first sampling so that `last` falls on 0, 62, 63, 64, 255, 256 and n-1: f_next then sits in
    the next wavefront, the next trip of the reduction, the next workgroup of the sampling pass."""
    ctx = dam1
    dy = F(0.0011)
    x, Y0 = 0.35, 0.5
    first = ctx.gauges([[x, Y0, 0.0, dy, 1500]], 0.5)[0]
    L0 = int(first["last"])
    assert first["inside"] == L0 - int(first["first"]) + 1 and L0 >= 300 and L0 < 1499, first  # a solid column of water under the surface
    ys = gr.gauge_points(F(x), F(Y0), F(0.0), dy, 1500)[:, 1]
    cols = []
    for target, n in ((0, 300), (62, 300), (63, 300), (64, 300), (255, 300), (256, 300), (299, 300), (63, 64), (255, 256)):
        y0 = ys[L0 - target]
        for _ in range(4):  # (the fp32 points of the shifted column are not those of the first: settle on the target)
            last = int(ctx.gauges([[x, y0, 0.0, dy, n]], 0.5)[0]["last"])
            if last == target:
                break
            y0 = F(y0 + F(last - target) * dy)
        assert last == target, (target, n, last)
        rec, val = check_call(ctx, [[x, y0, 0.0, dy, n]], 0.5, what="last = %d of %d" % (target, n))
        assert rec[0]["last"] == target and rec[0]["inside"] == target + 1
        assert (rec[0]["t"] == 0 and np.isnan(rec[0]["f_next"])) if target == n - 1 else (0 <= rec[0]["t"] <= 1 and rec[0]["f_next"] == val[target + 1])
        cols.append([x, y0, 0.0, dy, n])
    rec, _ = check_call(ctx, cols, 0.5, what="the edge columns in one call")
    assert rec["last"].tolist() == [0, 62, 63, 64, 255, 256, 299, 63, 255]
    # iso set to the bits of one sampled value: equality counts as inside
    _, val = ctx.gauges([[x, Y0, 0.0, dy, 1500]], 0.5, values=True)
    j = L0 + 1
    assert 0 < val[j] < 0.5
    rec, _ = check_call(ctx, [[x, Y0, 0.0, dy, 1500]], float(val[j]), what="iso = a sampled value")
    assert rec[0]["last"] >= j and not gr.same_bytes(gr.reduce32(val, [[x, Y0, 0.0, dy, 1500]], val[j], "strict_greater"), rec)
    if rec[0]["last"] == j:
        assert rec[0]["t"] == 0 and rec[0]["y"] == ys[j]


def test_a_column_through_the_splash_has_a_gap(dam400):
    ctx, _ = dam400
    cols = [[x, 0.0, 0.0, 0.005, 400] for x in np.linspace(0.02, 1.98, 99)]
    rec, _ = check_call(ctx, cols, 0.5, what="99 columns at step 400")
    wet = rec["inside"] > 0
    gap = wet & (rec["inside"] < rec["last"] - rec["first"] + 1)
    assert wet.sum() > 60 and gap.any(), "no column with a bubble or a detached splash at step 400"


# ---- 3. the contour on the device -------------------------------------------------------------------------------------------------------------
def test_vertical_gauges_lie_on_the_contour(dam400):
    ctx, _ = dam400
    seen = 0
    for kind, field in ((y.KERNEL_WENDLAND_C2, "fraction"), (y.KERNEL_POLY6, "density")):
        for g in RAYS[:5] + [[0.61, 0.013, 0.0, 0.0071, 211]]:
            rec = ctx.gauges([g], ISO[field], field, kind)[0]
            if not 0 <= rec["last"] < g[4] - 1:
                continue
            c = ctx.contour((F(g[0]), F(g[1])), (F(0.0123), F(g[3])), (g[4], 2), iso=ISO[field], field=field, kind=kind)
            ends = {e.tobytes() for e in c["segments"][c["cell"] == rec["last"]].reshape(-1, 2)}
            assert np.array([rec["x"], rec["y"]], F).tobytes() in ends, (g, rec)
            seen += 1
    assert seen >= 6


# ---- 4-6. device pointers, memory behind the arrays, repeated calls ------------------------------------------------------------------------
def test_device_pointers_canaries_and_repeated_calls(dam400):
    import torch

    ctx, _ = dam400
    g = y._gauge_array(RAYS)
    total = int(g["n"].sum())
    rec, val = ctx.gauges(RAYS, 0.5, values=True)
    rec2, val2 = ctx.gauges(RAYS, 0.5, values=True)
    assert gr.same_bytes(rec, rec2) and gr.same_bytes(val, val2)  # two calls on one state return the same bytes
    out = torch.full((len(g) * 32 + 64,), 0xCD, dtype=torch.uint8, device="cuda")
    dval = torch.full((total + 16,), -7.0, dtype=torch.float32, device="cuda")
    for _ in range(2):
        o, v = ctx.gauges(RAYS, 0.5, values=dval[:total], out=out[:len(g) * 32])
        assert o.cpu().numpy().tobytes() == rec.tobytes() and np.array_equal(words(v.cpu().numpy()), words(val))
        assert (out[len(g) * 32:].cpu().numpy() == 0xCD).all() and (dval[total:].cpu().numpy() == -7.0).all()
    o = ctx.gauges(RAYS, 0.5, out=out[:len(g) * 32])  # (the values go to the scratch)
    assert o.cpu().numpy().tobytes() == rec.tobytes()
    # an `out` that is 4-byte aligned only
    odd = torch.full((len(g) * 32 + 8,), 0xCD, dtype=torch.uint8, device="cuda")
    o = ctx.gauges(RAYS, 0.5, out=odd[4:4 + len(g) * 32])
    assert o.cpu().numpy().tobytes() == rec.tobytes() and (odd[:4].cpu().numpy() == 0xCD).all() and (odd[-4:].cpu().numpy() == 0xCD).all()
    # host path: canaries behind the host arrays
    hrec = np.full(len(g) * 8 + 16, 0xABABABAB, np.uint32)
    hval = np.full(total + 16, -7.0, F)
    assert ctx.L.sphx_gauge_levels(ctx.h, g.ctypes.data, len(g), 0, 0, 0.5, 0, hrec.ctypes.data, hval.ctypes.data) == _lib.OK
    assert hrec[:len(g) * 8].tobytes() == rec.tobytes() and (hrec[len(g) * 8:] == 0xABABABAB).all()
    assert np.array_equal(words(hval[:total]), words(val)) and (hval[total:] == -7.0).all()
    with pytest.raises(ValueError):
        ctx.gauges(RAYS, 0.5, out=out)  # the wrong size


# ---- 7. state rules and argument errors ---------------------------------------------------------------------------------------------------------
def test_state_rules_and_argument_errors():
    ctx, twin = scene_ctx(), scene_ctx()
    L, h, bad = ctx.L, ctx.h, _lib.ERR_INVALID_ARGUMENT
    g1 = y._gauge_array([[0.2, 0.0, 0.0, 0.01, 100]])
    rec = np.zeros(4, y.GAUGE_REC_DTYPE)
    pts = np.zeros((4, 2), F)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    msg = lambda: L.sphx_last_error(h).decode()

    def levels(g=g1, n=None, kind=0, field=0, iso=0.5, flags=0, out=rec, c=ctx):
        return c.L.sphx_gauge_levels(c.h, p(g) if g is not None else None, len(g) if n is None else n, kind, field, iso, flags,
                                     p(out) if out is not None else None, None)

    def record(g=g1, n=None, xy=pts, m=4, kind=0, field=0, iso=0.5, max_frames=4, every=1, c=ctx):
        return c.L.sphx_probe_record(c.h, p(xy) if xy is not None else None, m, p(g) if g is not None else None, len(g) if n is None else n, kind,
                                     field, iso, max_frames, every)

    def err(rc, code, needle):
        assert rc == code and needle in msg(), (rc, code, needle, msg())

    def sampling_says():
        d = np.zeros(4, F)
        o = _lib.SphxSampleOut(density=d.ctypes.data)
        assert L.sphx_sample_points(h, p(pts), 4, 0, 0, C.byref(o)) == _lib.ERR_NOT_READY
        return msg().split(": ", 1)[1]

    # when allowed: sampling's refusals, with sampling's message
    want = sampling_says()
    err(levels(), _lib.ERR_NOT_READY, want)  # after upload
    assert record() == _lib.OK  # ... but a recording may be switched on before the first step
    assert ctx.probe_status() == dict(m_points=4, n_gauges=1, recording=1, max_frames=4, every=1, frames=0, dropped=0)
    assert record(max_frames=0) == _lib.OK
    ctx.update_neighborhood(), twin.update_neighborhood()
    want = sampling_says()
    err(levels(), _lib.ERR_NOT_READY, want)
    assert "sphx_update_densities" in want
    ctx.update_densities(y.KERNEL_WENDLAND_C2), twin.update_densities(y.KERNEL_WENDLAND_C2)
    assert levels() == _lib.OK
    ta, tb = y.TimeManager(), y.TimeManager()
    for _ in range(2):
        dfsph_step(ctx, ta), dfsph_step(twin, tb)
    assert levels() == _lib.OK and rec[0]["inside"] > 0
    # argument errors on a ready context; the message names the argument
    err(levels(out=None), bad, "out")
    err(levels(g=None, n=1), bad, "gauges")
    big = np.zeros(_lib.GAUGE_MAX + 1, y.GAUGE_DTYPE)
    big["n"] = 1
    err(levels(g=big, out=np.zeros(_lib.GAUGE_MAX + 1, y.GAUGE_REC_DTYPE)), bad, "SPHX_GAUGE_MAX")
    err(record(g=big), bad, "SPHX_GAUGE_MAX")
    for n in (0, 2 ** 20 + 1):
        err(levels(g=y._gauge_array([[0.2, 0.0, 0.0, 0.01, n]])), bad, "n == 0 or n > 2^20")
        err(record(g=y._gauge_array([[0.2, 0.0, 0.0, 0.01, n]])), bad, "n == 0 or n > 2^20")
    err(levels(g=y._gauge_array([[0.2, 0.0, 0.0, 0.01, 2 ** 20]] * 17), out=np.zeros(17, y.GAUGE_REC_DTYPE)), bad, "2^24")
    for k in range(4):
        for x in (np.nan, np.inf, -np.inf):
            row = [0.2, 0.0, 0.0, 0.01, 100]
            row[k] = x
            err(levels(g=y._gauge_array([row])), bad, "non-finite")
            err(record(g=y._gauge_array([row])), bad, "non-finite")
    for iso in (np.nan, np.inf, -np.inf):
        err(levels(iso=iso), bad, "iso")
        err(record(iso=iso), bad, "iso")
    for kind in (3, -1):
        err(levels(kind=kind), bad, "kernel_kind")
        err(record(kind=kind), bad, "kernel_kind")
    for field in (2, -1):
        err(levels(field=field), bad, "field")
        err(record(field=field), bad, "field")
    for flags in (2, 0x80000000, 3):
        err(levels(flags=flags), bad, "flags")
    assert levels(g=None, n=0) == _lib.OK  # n_gauges == 0 succeeds
    assert levels(g=y._gauge_array([[1.0, 1.0, 0.0, 0.0, 5], [1.0, 1.0, -0.01, -0.01, 5]])) == _lib.OK  # zero and negative steps are legal
    with pytest.raises(ValueError):
        ctx.gauges(RAYS, field="pressure")
    # the recorder's arguments
    err(record(every=0), bad, "every")
    err(record(g=None, n=0, xy=None, m=0), bad, "m_points + n_gauges")
    err(record(m=2 ** 20), bad, "m_points")
    err(record(xy=None, m=4), bad, "points_xy")
    err(record(max_frames=(64 << 20) // (5 * 32) + 1), _lib.ERR_CAPACITY, "64 MiB")
    err(record(g=None, n=0, m=1, max_frames=(64 << 20) // 32 + 1), _lib.ERR_CAPACITY, "64 MiB")
    err(record(max_frames=0xFFFFFFFF), _lib.ERR_CAPACITY, "64 MiB")
    assert record(g=None, n=0, m=1, max_frames=(64 << 20) // 32) == _lib.OK  # exactly 64 MiB
    assert ctx.probe_status()["recording"] == 1 and record(max_frames=0, every=0, kind=9) == _lib.OK  # (stopping takes any argument)
    assert ctx.probe_status() == dict(m_points=0, n_gauges=0, recording=0, max_frames=0, every=0, frames=0, dropped=0)
    assert L.sphx_probe_get_status(h, None) == bad
    assert record(max_frames=2) == _lib.OK
    err(L.sphx_probe_read(h, 0, 1, None, p(rec), None), bad, "first_frame + n_frames")
    assert L.sphx_probe_read(h, 0, 0, None, None, None) == _lib.OK
    dfsph_step(ctx, ta), dfsph_step(twin, tb)
    err(L.sphx_probe_read(h, 1, 1, None, p(rec), None), bad, "first_frame + n_frames")
    err(L.sphx_probe_read(h, 0xFFFFFFFF, 2, None, p(rec), None), bad, "first_frame + n_frames")
    assert L.sphx_probe_read(h, 0, 1, None, p(rec), None) == _lib.OK and gr.same_bytes(rec[:1], ctx.gauges(g1))  # (the other pointers may be NULL)
    assert L.sphx_probe_read(h, 0, 1, None, None, None) == _lib.OK
    assert record(max_frames=0) == _lib.OK
    # inside a step, for both solvers
    va, vb = ctx.step_begin(ta.simulation_step()), twin.step_begin(tb.simulation_step())
    err(levels(), _lib.ERR_NOT_READY, "step_begin")
    err(record(), _lib.ERR_NOT_READY, "step_begin")
    err(L.sphx_probe_read(h, 0, 0, None, None, None), _lib.ERR_NOT_READY, "step_begin")
    dt = y.duration_as_secs_f32(ta.update_simulation_step(DIAM, va))
    assert va == vb and y.duration_as_secs_f32(tb.update_simulation_step(DIAM, vb)) == dt
    assert ctx.step_finish(dt) == twin.step_finish(dt)
    w = scene_ctx()
    w.wcsph_step_begin(F(1e-4))
    assert levels(c=w) == _lib.ERR_NOT_READY and record(c=w) == _lib.ERR_NOT_READY
    # after all those refusals the context still steps like its twin
    for _ in range(3):
        assert dfsph_step(ctx, ta) == dfsph_step(twin, tb)
    assert ctx.state_digest() == twin.state_digest() and ctx.last_flags() == twin.last_flags()
    # a tile context
    tc = y.SphxContext()
    assert tc.L.sphx_tile_configure(tc.h, 0, 0, 65536, 4, 0, 0) == _lib.OK
    for rc in (levels(c=tc), record(c=tc), tc.L.sphx_probe_read(tc.h, 0, 0, None, None, None)):
        assert rc == bad and "not available on a tile context" in tc.L.sphx_last_error(tc.h).decode()


# ---- 8. the recorder against one-shot calls -------------------------------------------------------------------------------------------------
REC_GAUGES = RAYS[:3] + RAYS[5:7]  # three columns, the bed, a downward ray


@pytest.fixture(scope="module")
def twin40():
    """40 steps of the reference scene through DFSPHSolver, one at a time, with one-shot calls after every step"""
    w = y.FluidParticleWorld()
    w.reset_fluid(1.0)
    b, tb = y.DFSPHSolver(w), y.TimeManager()
    stats, pts, gau = [], [], []
    for _ in range(40):
        stats.append(b.simulation_step(w, tb, sync_world=False))
        ctx = b.context()
        pts.append(ctx.sample(POINTS))
        gau.append(ctx.gauges(REC_GAUGES, 0.5))
    return stats, pts, gau


@pytest.mark.parametrize("every", [1, 3])
@pytest.mark.parametrize("one_call", [False, True])
def test_recorder_against_one_shot_calls(twin40, every, one_call):
    stats, pts, gau = twin40
    w = y.FluidParticleWorld()
    w.reset_fluid(1.0)
    a, ta = y.DFSPHSolver(w), y.TimeManager()
    ctx = a.context()
    ctx.probe_record(POINTS, REC_GAUGES, max_frames=40, every=every)  # (before the first step)
    got = a.simulation_steps(w, ta, 40, sync_world=False) if one_call else [a.simulation_step(w, ta, sync_world=False) for _ in range(40)]
    assert got == stats
    st = ctx.probe_status()
    assert st == dict(m_points=8, n_gauges=5, recording=1, max_frames=40, every=every, frames=40 // every, dropped=0)
    fr = ctx.probe_frames()
    assert fr["points"].shape == (40 // every, 8) and fr["gauges"].shape == (40 // every, 5) and fr["info"].dtype == y.STATS_FRAME_DTYPE
    steps = list(range(every, 41, every))
    assert fr["info"]["step"].tolist() == steps and (fr["info"]["n"] == 4050).all()
    assert fr["info"]["dt"].tobytes() == np.array([stats[s - 1]["dt"] for s in steps], F).tobytes()
    for f, s in enumerate(steps):
        assert gr.same_bytes(fr["gauges"][f], gau[s - 1]), "gauges of frame %d against the call after step %d" % (f, s)
        for name in ("density", "fraction", "velocity", "count"):
            assert np.array_equal(words(fr["points"][f][name]), words(pts[s - 1][name])), (f, s, name)
        assert not fr["points"][f]["reserved"].any()
    assert not gr.same_bytes(fr["gauges"][0], fr["gauges"][-1]) and (fr["points"]["count"][:, :6] > 0).any()
    one = ctx.probe_frames(1, 2)
    assert all(gr.same_bytes(one[k], fr[k][1:3]) for k in ("points", "gauges", "info"))


# ---- 9. the recorder's bookkeeping ------------------------------------------------------------------------------------------------------------
def test_recorder_bookkeeping_and_lifetime():
    ctx, timer = scene_ctx(), y.TimeManager()
    assert ctx.probe_status() == dict(m_points=0, n_gauges=0, recording=0, max_frames=0, every=0, frames=0, dropped=0)
    ctx.probe_record(POINTS, REC_GAUGES, max_frames=3, every=2)
    dts = [dfsph_step(ctx, timer) for _ in range(9)]
    assert ctx.probe_status() == dict(m_points=8, n_gauges=5, recording=1, max_frames=3, every=2, frames=3, dropped=1)
    fr = ctx.probe_frames()
    assert fr["info"]["step"].tolist() == [2, 4, 6] and fr["info"]["dt"].tobytes() == np.array([dts[1], dts[3], dts[5]], F).tobytes()
    # a failed step takes no frame and does not count; a new record discards the old recording
    ctx.probe_record(None, REC_GAUGES, max_frames=4, every=2)
    assert ctx.probe_status() == dict(m_points=0, n_gauges=5, recording=1, max_frames=4, every=2, frames=0, dropped=0)
    dfsph_step(ctx, timer)
    ctx.step_begin(timer.simulation_step())
    with pytest.raises(y.SphxError):
        ctx.step_finish(F(-1.0))
    assert ctx.probe_status()["frames"] == 0
    dt = dfsph_step(ctx, timer)
    fr = ctx.probe_frames()
    assert fr["points"].shape == (1, 0) and fr["gauges"].shape == (1, 5) and fr["info"]["step"].tolist() == [2] and fr["info"]["dt"][0] == F(dt)
    assert gr.same_bytes(fr["gauges"][0], ctx.gauges(REC_GAUGES))
    # points alone; max_frames = 0 stops and frees
    ctx.probe_record(POINTS, None, max_frames=2)
    dfsph_step(ctx, timer)
    fr = ctx.probe_frames()
    assert fr["gauges"].shape == (1, 0) and np.array_equal(words(fr["points"][0]["fraction"]), words(ctx.sample(POINTS)["fraction"]))
    ctx.probe_record(max_frames=0)
    assert ctx.probe_status() == dict(m_points=0, n_gauges=0, recording=0, max_frames=0, every=0, frames=0, dropped=0)
    dfsph_step(ctx, timer)
    assert ctx.probe_status()["frames"] == 0
    with pytest.raises(y.SphxError):
        ctx.probe_frames(0, 1)
    # the recording belongs to the context: append, remove, upload and load_state leave it alone
    ctx.probe_record(POINTS, REC_GAUGES, max_frames=8)
    dfsph_step(ctx, timer)
    extra = (np.array([1.2, 1.0], F) + np.stack(np.meshgrid(np.arange(20), np.arange(20)), -1).reshape(-1, 2).astype(F) * F(0.0111)).astype(F)
    ctx.append(extra, np.full_like(extra, -1.0))
    dfsph_step(ctx, timer)
    removed = ctx.remove((0.2, 0.4, 0.7, 0.9))
    assert removed > 0
    dfsph_step(ctx, timer)
    st = ctx.probe_status()
    assert (st["recording"], st["frames"], st["dropped"]) == (1, 3, 0)
    fr = ctx.probe_frames()
    assert fr["info"]["n"].tolist() == [4050, 4450, 4450 - removed] and gr.same_bytes(fr["gauges"][2], ctx.gauges(REC_GAUGES))
    blob = ctx.save_state()
    ctx.upload(dam_break(1.0)[0][:1000])
    ctx.load_state(blob)
    after = ctx.probe_frames()
    assert ctx.probe_status()["frames"] == 3 and all(gr.same_bytes(after[k], fr[k]) for k in fr)
    dfsph_step(ctx, timer)
    assert ctx.probe_status()["frames"] == 4 and gr.same_bytes(ctx.probe_frames(3, 1)["gauges"][0], ctx.gauges(REC_GAUGES))
    # a WCSPH step over zero fluid particles runs no build: no frame, counted in `dropped`; WCSPH frames otherwise
    w = y.SphxContext()
    w.set_boundary(dam_break(1.0)[1])
    w.upload(np.zeros((0, 2), F))
    w.probe_record(POINTS, REC_GAUGES, max_frames=4)
    tw = y.TimeManager(cfl_factor=0.2)
    wcsph_step(w, tw)
    assert w.probe_status() == dict(m_points=8, n_gauges=5, recording=1, max_frames=4, every=1, frames=0, dropped=1)
    w.upload(dam_break(1.0)[0])
    wcsph_step(w, tw)
    assert (w.probe_status()["frames"], w.probe_status()["dropped"]) == (1, 1)
    fr = w.probe_frames()
    assert fr["info"]["step"].tolist() == [2] and gr.same_bytes(fr["gauges"][0], w.gauges(REC_GAUGES))


# ---- 10. no side effects ----------------------------------------------------------------------------------------------------------------------
def _run(n_steps, probing, wcsph, run_ahead):
    import torch

    old = os.environ.get("SPHX_RUN_AHEAD")
    os.environ["SPHX_RUN_AHEAD"] = "1" if run_ahead else "0"
    try:
        ctx = scene_ctx()
    finally:
        if old is None:
            del os.environ["SPHX_RUN_AHEAD"]
        else:
            os.environ["SPHX_RUN_AHEAD"] = old
    timer = y.TimeManager(cfl_factor=0.2) if wcsph else y.TimeManager()
    log = []
    if probing:
        ctx.probe_record(POINTS, RAYS, max_frames=n_steps // 2, every=2)
        out = torch.zeros(len(RAYS) * 32, dtype=torch.uint8, device="cuda")
    for s in range(n_steps):
        (wcsph_step if wcsph else dfsph_step)(ctx, timer, log)
        if probing:
            ctx.gauges(RAYS, 0.5)
            if s % 3 == 0:
                ctx.gauges(RAYS[:6], 60.0, "density", y.KERNEL_POLY6, values=True)
                ctx.gauges(RAYS, 0.5, out=out)
            assert ctx.last_flags() == log[-1][3]
    if probing:
        assert ctx.probe_status()["frames"] == n_steps // 2
    return log, ctx.state_digest(), ctx.download()


@pytest.mark.parametrize("wcsph, steps, run_ahead", [(False, 100, True), (False, 100, False), (True, 30, True)])
def test_recording_and_calls_have_no_side_effects(wcsph, steps, run_ahead):
    log_a, dig_a, a = _run(steps, False, wcsph, run_ahead)
    log_b, dig_b, b = _run(steps, True, wcsph, run_ahead)
    assert log_b == log_a  # vmax, the timer's step, every sphx_step_stats field, sphx_last_flags
    assert dig_a == dig_b
    for k in ("pos", "vel", "density", "ids"):
        assert np.array_equal(words(a[k]), words(b[k])), k


# ---- 11. the harness --------------------------------------------------------------------------------------------------------------------------
def test_harness_gauge_out(tmp_path):
    steps, every = 12, 2
    xs = [0.05, 0.2, 0.35, 1.0]
    path = tmp_path / "gauges.csv"
    base = [HARNESS, "--scale", "1", "--steps", str(steps), "--warmup", "0", "--gauges", ",".join(map(str, xs))]
    plain = subprocess.run(base, capture_output=True, text=True, timeout=600)
    out = subprocess.run(base + ["--gauge-out", str(path), "--gauge-every", str(every)], capture_output=True, text=True, timeout=600)
    assert plain.returncode == 0 and out.returncode == 0, out.stderr
    res, res0 = json.loads(out.stdout.strip().splitlines()[-1]), json.loads(plain.stdout.strip().splitlines()[-1])
    assert res["gauge_frames"] == steps // every and "gauge_frames" not in res0
    assert res["gauge_elevations"] == res0["gauge_elevations"] and res["state_fnv1a"] == res0["state_fnv1a"]  # unchanged by the recording
    lines = path.read_text().splitlines()
    assert lines[0] == "step,dt,gauge,first,last,inside,x,y" and len(lines) == 1 + (steps // every) * len(xs)
    # the same run through Python, with the recorder on the same columns
    w = y.FluidParticleWorld()
    w.reset_fluid(1.0)
    dy = float(w.properties()["particle_radius"]) / 2.0
    ny = int(np.floor(2.5 / dy)) + 1
    ctx = y.SphxContext()
    ctx.set_boundary(w.boundary_particles)
    ctx.upload(w.positions)
    ctx.probe_record(None, [[x, 0.0, 0.0, dy, ny] for x in xs], max_frames=steps // every, every=every)
    timer = y.TimeManager()
    for _ in range(steps):
        timer.on_step_started()  # the harness advances the clock like simulation_frame_loop does (timemanager.rs:244-247)
        dfsph_step(ctx, timer)
    fr = ctx.probe_frames()
    assert fr["gauges"].shape == (steps // every, len(xs)) and (fr["gauges"]["inside"][:, 1:3] > 0).all()  # (the block stands over x = 0.2 and 0.35)
    for k, ln in enumerate(lines[1:]):
        step, dt, gauge, first, last, inside, x, yv = ln.split(",")
        f, g = divmod(k, len(xs))
        r = fr["gauges"][f, g]
        assert (int(step), int(gauge), int(first), int(last), int(inside)) == (fr["info"]["step"][f], g, r["first"], r["last"], r["inside"]), ln
        assert F(dt) == fr["info"]["dt"][f]
        for got, want in ((x, r["x"]), (yv, r["y"])):
            assert (np.isnan(F(got)) and np.isnan(want)) or F(got) == want, ln
    # malformed options exit with status 2
    for bad in (["--gauge-out", str(path)], ["--gauges", "0.1", "--gauge-out", ""], ["--gauges", "0.1", "--gauge-every", "2"],
                ["--gauges", "0.1", "--gauge-out", str(path), "--gauge-every", "0"]):
        r = subprocess.run([HARNESS, "--scale", "1", "--steps", "1", "--warmup", "0"] + bad, capture_output=True, text=True, timeout=120)
        assert r.returncode == 2, bad
