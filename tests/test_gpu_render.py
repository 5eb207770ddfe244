"""Rendering on the device (sphx_render): rgba and owner bit-equal to the float32 restatement of the contract
(tests/render_reference.py) over states, views, radii, odd sizes and paths; hostile positions; the state rules and every argument
error of include/sphx.h; no side effects on a run; a 1 M-particle frame; the harness's recording mode.

The cross product of states x views x outputs x paths is sampled, not exhausted, to keep the file at about a minute: the state after
100 DFSPH steps gets every view, on the host path with both outputs and on the device-pointer path; the other states (upload only,
1 and 10 DFSPH steps, 30 WCSPH steps) get the whole scene at 640 x 360, the zoom onto the median particle and the 60 pixels-per-unit
view with min_pixel_radius 0.75; "rgba only" and "owner only" are checked on three views of the 100-step state on both paths."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import render_reference as rr
import yasph2d_amd as y
from util import dam_break
from yasph2d_amd import _lib

pytestmark = pytest.mark.gpu

F = np.float32
DIAM = F(0.01)
HARNESS = os.path.join(os.path.dirname(os.path.abspath(y.__file__)), "sphx_harness")


def dfsph_steps(ctx, timer, k):
    for _ in range(k):
        vmax = ctx.step_begin(timer.simulation_step(), timer.law(DIAM))
        ctx.step_finish(y.duration_as_secs_f32(timer.update_simulation_step(DIAM, vmax)))


def wcsph_steps(ctx, timer, k):
    for _ in range(k):
        vmax = ctx.wcsph_step_begin(timer.simulation_step())
        ctx.wcsph_step_finish(y.duration_as_secs_f32(timer.update_simulation_step(DIAM, vmax)))


def scene_ctx(scale=1.0, **kw):
    pos, bnd = dam_break(scale)
    ctx = y.SphxContext(**kw)
    ctx.set_boundary(bnd)
    ctx.upload(pos)
    return ctx


def state_of(ctx):
    d = ctx.download(density=False, ids=False)
    return dict(pos=d["pos"], vel=d["vel"], boundary=ctx.download_boundary()[0])


def radius_of(ctx):
    return F(ctx.params.particle_radius)


def device_render(ctx, view, rgba=True, owner=True):
    """the device-pointer path into pre-filled torch tensors (an unwritten pixel shows)"""
    import torch

    h, w = view.height, view.width
    img = torch.full((h, w, 4), 7, dtype=torch.uint8, device="cuda") if rgba else None
    own = torch.full((h, w), -7, dtype=torch.int32, device="cuda") if owner else None
    r = ctx.render(**view.fields(), out=img, rgba=rgba, owner=own if owner else False)
    out = {}
    if rgba:
        out["rgba"] = img.cpu().numpy()
    if owner:
        assert (r if not rgba else r[1]) is own
        out["owner"] = own.cpu().numpy().view(np.uint32)
    return out


def assert_image(got, ref, what):
    for k, a in got.items():
        b = ref[k]
        assert a.shape == b.shape and a.dtype == b.dtype, (what, k, a.shape, b.shape, a.dtype, b.dtype)
        if not np.array_equal(a, b):
            bad = np.argwhere((a != b).reshape(a.shape[0], a.shape[1], -1).any(-1))
            raise AssertionError("%s: %s differs at %d of %d pixels, first (row %d, column %d): %s vs %s" % (
                what, k, len(bad), a.shape[0] * a.shape[1], bad[0][0], bad[0][1], a[tuple(bad[0])], b[tuple(bad[0])]))


def check_view(ctx, st, view, what, device=True, singles=False, mode="full"):
    ref = rr.render32(st, view, radius_of(ctx), mode=mode)
    img, own = ctx.render(**view.fields(), owner=True)
    assert_image(dict(rgba=img, owner=own), ref, what + " host")
    if device:
        assert_image(device_render(ctx, view), ref, what + " device pointers")
    if singles:
        assert_image(dict(rgba=ctx.render(**view.fields())), ref, what + " host rgba only")
        assert_image(dict(owner=ctx.render(**view.fields(), rgba=False, owner=True)), ref, what + " host owner only")
        assert_image(device_render(ctx, view, owner=False), ref, what + " device rgba only")
        assert_image(device_render(ctx, view, rgba=False), ref, what + " device owner only")
    return ref


def median_of(st):
    return (F(np.median(st["pos"][:, 0])), F(np.median(st["pos"][:, 1])))


def core_views(st):
    return [("whole 640x360", rr.fit(640, 360)), ("zoom on the median particle", rr.View(640, 360, median_of(st), 3000.0)),
            ("60 px per unit, min_pixel_radius 0.75", rr.View(160, 120, (0.95, 0.7), 60.0, min_pixel_radius=0.75))]


def all_views(st):
    m = median_of(st)
    vs = core_views(st) + [("whole 1920x1080", rr.fit(1920, 1080))]
    for ppu in (20.0, 60.0):
        for mpr in (0.0, 0.75, 4.0):
            vs.append(("%g px per unit, min_pixel_radius %g" % (ppu, mpr), rr.View(160, 120, (0.95, 0.7), ppu, min_pixel_radius=mpr)))
    for radius in (0.015, 0.02):
        vs.append(("whole 640x360 radius %g" % radius, rr.fit(640, 360, radius=radius)))
    vs.append(("zoom, radius 0.02, min_pixel_radius 4", rr.View(320, 200, m, 1500.0, radius=0.02, min_pixel_radius=4.0)))
    for (w, h) in ((1, 1), (1, 777), (333, 1), (17, 13)):
        vs.append(("%d x %d on the median particle" % (w, h), rr.View(w, h, m, 400.0, radius=0.015)))
    vs.append(("1 x 1 far from everything", rr.View(1, 1, (5.0, 5.0), 400.0)))
    vs.append(("a view that contains nothing", rr.View(320, 200, (50.0, 50.0), 300.0)))
    vs.append(("half outside the scene", rr.View(640, 360, (0.0, 0.0), 300.0)))
    vs.append(("other colours and speed scale", rr.fit(320, 180, speed_scale=0.37, background=(1, 2, 3, 4), boundary=(250, 0, 9, 77))))
    return vs


# ------------------------------------------------------------------------------------------------------------------------- bit equality
def test_reference_scene_bit_exact_over_states_and_views():
    ctx = scene_ctx()
    timer = y.TimeManager()
    done = 0
    for steps in (0, 1, 10, 100):
        dfsph_steps(ctx, timer, steps - done)
        done = steps
        st = state_of(ctx)
        views = all_views(st) if steps == 100 else core_views(st)
        for i, (name, view) in enumerate(views):
            ref = check_view(ctx, st, view, "%d steps, %s" % (steps, name), singles=steps == 100 and i < 3)
            if name == "whole 640x360":
                fluid = ref["owner"] < rr.BOUNDARY
                assert fluid.mean() >= 0.02 and (ref["owner"] == rr.BOUNDARY).mean() >= 0.02 and (ref["owner"] == rr.NONE).mean() >= 0.02
                if steps == 100:  # every channel of the heat map is in use
                    assert all((ref["rgba"][fluid][:, k] > 0).any() for k in range(3))
            if name == "a view that contains nothing":
                assert (ref["owner"] == rr.NONE).all() and (ref["rgba"] == rr.BACKGROUND).all()
    # rendering the same state twice gives the same bytes
    v = rr.fit(640, 360, radius=0.015)
    a, b = ctx.render(**v.fields(), owner=True), ctx.render(**v.fields(), owner=True)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    # the default view is the app's camera on a 1920 x 1080 screen, and a SphxRenderView is taken as it is
    img = ctx.render()
    assert img.shape == (1080, 1920, 4) and np.array_equal(img, ctx.render(y.render_fit(1920, 1080)))
    assert np.array_equal(ctx.render(y.render_fit(640, 360), radius=0.015), a[0])


def test_wcsph_state_bit_exact():
    ctx = scene_ctx()
    wcsph_steps(ctx, y.TimeManager(cfl_factor=0.2), 30)
    st = state_of(ctx)
    for name, view in core_views(st):
        check_view(ctx, st, view, "30 WCSPH steps, " + name)


def test_hostile_positions_own_no_pixel():
    """Particles at +-1e30, +-3.4e38 and non-finite positions, NaN velocities, rendered without a step: SPHX_OK, they own nothing, the
    output is the restatement's."""
    pos, bnd = dam_break(1.0)
    pos = pos.copy()
    vel = np.zeros_like(pos)
    vel[::3] = (2.0, -1.0)
    finite = [(1e30, 0.5), (0.5, -1e30), (-1e30, 1e30), (3.4e38, 0.5), (0.5, -3.4e38), (-3.4e38, 3.4e38), (3.4e38, 3.4e38)]
    nonfinite = [(np.nan, 0.5), (0.5, np.nan), (np.inf, 0.5), (0.5, -np.inf), (-np.inf, np.inf), (np.nan, np.nan)]
    where = np.arange(0, 40 * 97, 97)
    ctx = y.SphxContext()
    ctx.set_boundary(bnd)
    hostile = finite + nonfinite
    try:
        p = pos.copy()
        p[where[:len(hostile)]] = np.array(hostile, F)
        vel[where[2:6]] = np.nan
        vel[5::1000] = (np.nan, 1.0)
        ctx.upload(p, vel)
    except y.SphxError:  # sphx_upload does not take non-finite positions: the finite ones remain
        hostile = finite
        p = pos.copy()
        p[where[:len(hostile)]] = np.array(hostile, F)
        ctx.upload(p, vel)
    st = state_of(ctx)
    with np.errstate(all="ignore"):
        bad = np.nonzero(~(np.abs(st["pos"]) < 1e20).all(axis=1))[0]
    assert len(bad) == len(hostile)
    for name, view in [("whole", rr.fit(640, 360)), ("radius h, min 4", rr.fit(320, 180, radius=0.02, min_pixel_radius=4.0)),
                       ("far out", rr.View(64, 64, (0.0, 0.0), 1e-3)), ("zoom", rr.View(320, 200, (0.3, 0.3), 2500.0))]:
        ref = check_view(ctx, st, view, "hostile, " + name)
        assert not np.isin(ref["owner"], bad).any()
    nanv = np.nonzero(np.isnan(st["vel"]).any(axis=1) & (np.abs(st["pos"]) < 1e20).all(axis=1))[0]
    ref = rr.render32(st, rr.fit(640, 360, radius=0.015), radius_of(ctx))
    hit = np.isin(ref["owner"], nanv)
    assert hit.any() and (ref["rgba"][hit] == (0, 0, 0, 255)).all()  # a NaN speed is black
    check_view(ctx, st, rr.fit(640, 360, radius=0.015), "hostile, NaN velocities")


# ---------------------------------------------------------------------------------------------------------------- rules and arguments
def _rc(ctx, view=None, flags=0, out=None, **fields):
    """sphx_render on a small view; view / out False = NULL; returns (status, message)"""
    v = y.render_fit(32, 16)
    for k, val in fields.items():
        if k == "center":
            v.center[0], v.center[1] = val
        else:
            setattr(v, k, val)
    buf = np.zeros(max(1, v.width * v.height), np.uint32) if v.width * v.height < 1 << 20 else np.zeros(1, np.uint32)
    o = _lib.SphxRenderOut(rgba=buf.ctypes.data) if out is None else out
    rc = ctx.L.sphx_render(ctx.h, None if view is False else C.byref(v), flags, None if o is False else C.byref(o))
    return rc, ctx.L.sphx_last_error(ctx.h).decode()


def test_state_rules_and_argument_errors():
    E, OK = _lib.ERR_INVALID_ARGUMENT, _lib.OK
    _, bnd = dam_break(1.0)
    # before any upload: the boundary over the background; without a boundary: the background
    ctx = y.SphxContext()
    assert (ctx.render(width=64, height=36) == rr.BACKGROUND).all()
    ctx.set_boundary(bnd)
    empty = dict(pos=np.zeros((0, 2), F), vel=np.zeros((0, 2), F), boundary=ctx.download_boundary()[0])
    ref = check_view(ctx, empty, rr.fit(640, 360), "no particles uploaded")
    assert (ref["owner"] == rr.BOUNDARY).any() and not (ref["owner"] < rr.BOUNDARY).any()
    ctx.upload(np.zeros((0, 2), F))
    check_view(ctx, empty, rr.fit(640, 360), "zero particles uploaded")
    # no boundary
    pos, _ = dam_break(1.0)
    nb = y.SphxContext()
    nb.upload(pos)
    st = dict(pos=pos, vel=np.zeros_like(pos), boundary=np.zeros((0, 2), F))
    ref = check_view(nb, st, rr.fit(640, 360, radius=0.015), "no boundary")
    assert not (ref["owner"] == rr.BOUNDARY).any() and (ref["owner"] < rr.BOUNDARY).any()
    # after an upload, after steps, not inside a step (either solver)
    ctx = scene_ctx()
    timer = y.TimeManager()
    assert _rc(ctx)[0] == OK
    dfsph_steps(ctx, timer, 2)
    assert _rc(ctx)[0] == OK
    ctx.step_begin(timer.simulation_step())
    rc, msg = _rc(ctx)
    assert rc == _lib.ERR_NOT_READY and "step_finish" in msg
    ctx.step_finish(y.duration_as_secs_f32(timer.update_simulation_step(DIAM, 0.0)))
    assert _rc(ctx)[0] == OK
    w = scene_ctx()
    t = y.TimeManager(cfl_factor=0.2)
    wcsph_steps(w, t, 1)
    assert _rc(w)[0] == OK
    w.wcsph_step_begin(t.simulation_step())
    assert _rc(w)[0] == _lib.ERR_NOT_READY
    # argument errors name the argument
    h = F(ctx.params.smoothing_length)
    assert ctx.L.sphx_render(None, None, 0, None) == E
    for kw, word in [(dict(view=False), "view"), (dict(out=False), "out"), (dict(out=_lib.SphxRenderOut()), "out"), (dict(flags=2), "flags"),
                     (dict(flags=0x80000001), "flags"),
                     (dict(pixel_per_world_unit=0.0), "pixel_per_world_unit"), (dict(pixel_per_world_unit=-3.0), "pixel_per_world_unit"),
                     (dict(pixel_per_world_unit=float("nan")), "pixel_per_world_unit"), (dict(pixel_per_world_unit=float("inf")), "pixel_per_world_unit"),
                     (dict(center=(float("nan"), 0.0)), "center"), (dict(center=(0.0, float("-inf"))), "center"),
                     (dict(radius=-0.001), "radius"), (dict(radius=float(np.nextafter(h, F(1)))), "radius"), (dict(radius=float("nan")), "radius"),
                     (dict(radius=float("inf")), "radius"),
                     (dict(min_pixel_radius=-0.5), "min_pixel_radius"), (dict(min_pixel_radius=4.001), "min_pixel_radius"),
                     (dict(min_pixel_radius=float("nan")), "min_pixel_radius"),
                     (dict(speed_scale=float("nan")), "speed_scale"), (dict(speed_scale=float("inf")), "speed_scale"),
                     (dict(width=1 << 14, height=1 << 14), "width"), (dict(width=1 << 28, height=1), "width"), (dict(width=0xFFFFFFFF, height=0xFFFFFFFF), "width")]:
        rc, msg = _rc(ctx, **kw)
        assert rc == E and word in msg, (kw, rc, msg)
    assert _rc(ctx, radius=float(h))[0] == OK and _rc(ctx, min_pixel_radius=4.0)[0] == OK and _rc(ctx, speed_scale=-1.0)[0] == OK
    # width * height == 0 is a successful no-op (once the arguments pass)
    assert _rc(ctx, width=0, height=5)[0] == OK and _rc(ctx, width=7, height=0)[0] == OK
    assert _rc(ctx, width=0, height=5, radius=-1.0)[0] == E
    assert ctx.render(width=0, height=4, pixel_per_world_unit=10.0).shape == (4, 0, 4)
    # the Python wrapper
    with pytest.raises(TypeError):
        ctx.render(widht=3)
    with pytest.raises(ValueError):
        ctx.render(rgba=False)
    with pytest.raises(y.SphxError) as e:
        ctx.render(width=8, height=8, radius=1.0)
    assert e.value.code == E and "radius" in str(e.value)
    # a tile context is refused
    tc = scene_ctx()
    assert tc.L.sphx_tile_configure(tc.h, 0, 0, 65536, 4, 0, 0) == OK
    rc, msg = _rc(tc)
    assert rc == E and "tile" in msg


# ------------------------------------------------------------------------------------------------------------------------ side effects
def _run(n_steps, render, wcsph=False):
    ctx = scene_ctx()
    timer = y.TimeManager(cfl_factor=0.2) if wcsph else y.TimeManager()
    st = state_of(ctx)  # (both runs download the state here)
    views = [v for _, v in core_views(st)]
    log = []
    if render:
        import torch

        img = torch.empty((360, 640, 4), dtype=torch.uint8, device="cuda")
    for _ in range(n_steps):
        if wcsph:
            vmax = ctx.wcsph_step_begin(timer.simulation_step())
            s = ctx.wcsph_step_finish(y.duration_as_secs_f32(timer.update_simulation_step(DIAM, vmax)))
        else:
            vmax = ctx.step_begin(timer.simulation_step(), timer.law(DIAM))
            s = ctx.step_finish(y.duration_as_secs_f32(timer.update_simulation_step(DIAM, vmax)))
        log.append((np.float32(vmax), timer.simulation_step_ns(), s["density_iterations"], s["divergence_iterations"], s["flags"], ctx.last_flags()))
        if render:
            ctx.render(**views[0].fields(), owner=True)
            ctx.render(**views[1].fields(), out=img)
            ctx.render(**views[2].fields(), rgba=False, owner=True)
            log[-1] += (ctx.last_flags(),)
    return log, ctx.download()


@pytest.mark.parametrize("wcsph", [False, True])
def test_renders_have_no_side_effects(wcsph):
    """40 steps with renders of all three views between every two steps equal 40 steps without, bit for bit."""
    log_a, a = _run(40, False, wcsph)
    log_b, b = _run(40, True, wcsph)
    assert [x[:6] for x in log_b] == log_a and all(x[6] == x[5] for x in log_b)
    for k in ("pos", "vel", "density", "ids"):
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k


# ------------------------------------------------------------------------------------------------------------------------------- scale
def test_one_million_particles_whole_scene():
    """BASELINE configs[1] (1 M particles) after 20 steps, the whole scene at 1920 x 1080 with min_pixel_radius 0.75, against the
    restatement with the particles' candidate pixels taken from their float64 screen positions (render_reference, mode "window")."""
    scale = float(np.sqrt(1.0e6 / 4050.0))
    ctx = scene_ctx(scale)
    dfsph_steps(ctx, y.TimeManager(), 20)
    st = state_of(ctx)
    view = rr.fit(1920, 1080, tuple(F(v) * F(scale) for v in rr.SCENE_RECT), min_pixel_radius=0.75)
    ref = check_view(ctx, st, view, "1 M particles", mode="window")
    assert (ref["owner"] < rr.BOUNDARY).mean() > 0.05
    # every fluid particle inside the image owns or shares a pixel: none falls between the pixel centres (it may be overdrawn)
    assert len(np.unique(ref["owner"][ref["owner"] < rr.BOUNDARY])) > 100000


# ----------------------------------------------------------------------------------------------------------------------------- harness
def test_harness_recording_matches_python(tmp_path):
    steps, fps, size = 60, 240.0, (320, 180)
    d = str(tmp_path / "rec")
    base = [HARNESS, "--scale", "1", "--steps", str(steps), "--warmup", "0"]
    out = subprocess.run(base + ["--record", d, "--record-fps", str(fps), "--record-size", "%dx%d" % size], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    res = json.loads(out.stdout.strip().splitlines()[-1])
    # the same run, driven from Python
    frame_ns = int(round(1e9 / fps))
    w = y.FluidParticleWorld()
    w.reset_fluid(1.0)
    ctx = y.SphxContext()
    ctx.set_boundary(w.boundary_particles)
    ctx.upload(w.positions)
    timer = y.TimeManager()
    timer.set_target_frame(frame_ns)
    view = rr.fit(size[0], size[1])
    frames = []
    for _ in range(steps):
        while max((len(frames) + 1) * frame_ns - timer.total_simulated_ns, 0) < timer.simulation_step_ns():
            frames.append(ctx.render(**view.fields()))
        timer.on_step_started()
        vmax = ctx.step_begin(timer.simulation_step(), timer.law(DIAM))
        ctx.step_finish(y.duration_as_secs_f32(timer.update_simulation_step(DIAM, vmax)))
    assert res["frames"] == len(frames) >= 3
    assert sorted(os.listdir(d), key=lambda s: int(s.split(".")[0])) == ["%d.ppm" % (k + 1) for k in range(len(frames))]
    head = b"P6\n%d %d\n255\n" % size
    for k, img in enumerate(frames):
        raw = open(os.path.join(d, "%d.ppm" % (k + 1)), "rb").read()
        assert len(raw) == len(head) + size[0] * size[1] * 3 and raw.startswith(head)
        assert raw[len(head):] == img[:, :, :3].tobytes(), "frame %d" % (k + 1)
    assert int(res["last_frame_fnv"], 16) == rr.fnv1a(frames[-1].tobytes())
    assert any((f != frames[0]).any() for f in frames[1:])  # the fluid moves
    # without --record the line is what it was; bad --record-* values exit with status 2 and a message
    plain = subprocess.run(base[:4] + ["2", "--warmup", "0"], capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0 and "frames" not in plain.stdout and "last_frame_fnv" not in plain.stdout
    for bad in (["--record", d, "--record-fps", "0"], ["--record", d, "--record-fps", "x"], ["--record", d, "--record-size", "320"],
                ["--record", d, "--record-size", "0x10"], ["--record", d, "--record-size", "3.5x10"], ["--record", d, "--record-size", "65536x65536"],
                ["--record", d, "--record-min-pixel-radius", "5"], ["--record", d, "--record-min-pixel-radius", "-1"], ["--record-fps", "60"],
                ["--record", ""], ["--record-size", "64x64"]):
        r = subprocess.run(base[:4] + ["1", "--warmup", "0"] + bad, capture_output=True, text=True, timeout=120)
        assert r.returncode == 2 and "--record" in r.stderr, bad
    r = subprocess.run(base[:4] + ["12", "--warmup", "0", "--record", d, "--record-size", "64x48", "--record-min-pixel-radius", "0.75", "--record-fps", "480"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and json.loads(r.stdout.strip().splitlines()[-1])["frames"] >= 1
