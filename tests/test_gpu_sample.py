"""Field sampling on the device (sphx_sample_points / sphx_sample_grid): the state rules and argument errors of include/sphx.h, bit
equality with the float32 restatement (tests/sample_reference.py) on every path, lattice = points, the float64 bound, consistency
with the solver's lists and densities, no side effects on a run, and the harness's gauges."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import sample_reference as sr
import yasph2d_amd as y
from util import dam_break, uniform_points
from yasph2d_amd import _lib

pytestmark = pytest.mark.gpu

F = np.float32
KINDS = (y.KERNEL_WENDLAND_C2, y.KERNEL_POLY6, y.KERNEL_SPIKY)
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
    d = ctx.download()
    assert not ctx.last_flags() & y.FLAG_STRAY_PARTICLES
    return dict(pos=d["pos"], vel=d["vel"], density=d["density"], boundary=ctx.download_boundary()[0], ids=d["ids"])


def consts_of(ctx):
    K = sr.Constants(ctx.params, ctx.constants())
    K0 = sr.Constants(ctx.params)  # (the restated derivation agrees with the device's constants)
    assert (K0.w_hinv, K0.w_norm, K0.p6_hsq, K0.p6_norm) == (K.w_hinv, K.w_norm, K.p6_hsq, K.p6_norm)
    return K


def probe_points(st, seed, h=0.02):
    rng = np.random.default_rng(seed)
    pos, bnd = st["pos"], st["boundary"]
    top = pos[np.argsort(pos[:, 1])[-200:]]
    pts = [pos[rng.choice(len(pos), 400, replace=False)],                                                   # at particles
           (pos[rng.choice(len(pos), 400, replace=False)] + rng.normal(0, h, (400, 2))).astype(F),          # bulk
           (top + rng.normal(0, h, top.shape)).astype(F),                                                   # free surface
           (bnd[rng.choice(len(bnd), 200, replace=False)] + rng.normal(0, h / 3, (200, 2))).astype(F),      # next to / inside walls
           sr.lattice_points(-0.07, -0.09, 0.0413, 0.0391, 57, 71),                                         # in and out of the fluid
           np.array([[1e6, 1e6], [-1e30, 0.5], [np.nan, 0.5], [0.5, np.nan], [np.inf, 0.5], [-np.inf, -np.inf], [-200.0, -200.0],
                     [3.4e38, -3.4e38]], F)]                                                                # far away, non-finite
    return np.concatenate(pts).astype(F)


def assert_bits(dev, ref, what):
    for f in dev:
        a, b = np.asarray(dev[f]), np.asarray(ref[f])
        if f != "count":
            a, b = a.astype(F).view(np.uint32), b.astype(F).view(np.uint32)
        assert a.shape == b.shape and np.array_equal(a, b), "%s: %s differs at %d points" % (what, f, int((a != b).any(-1).sum() if a.ndim > 1 else (a != b).sum()))


def grid_device(ctx, origin, spacing, shape, kind):
    """sphx_sample_grid with SPHX_SAMPLE_DEVICE_POINTERS into torch outputs (pre-filled: an unwritten entry shows)"""
    import torch

    ny, nx = shape
    outs = {f: torch.full((ny, nx, 2) if f == "velocity" else (ny, nx), -7, dtype=torch.int32 if f == "count" else torch.float32, device="cuda")
            for f in sr.FIELDS}
    o = y._out_struct(outs, lambda t: t.data_ptr())
    torch.cuda.current_stream().synchronize()
    rc = ctx.L.sphx_sample_grid(ctx.h, origin[0], origin[1], spacing[0], spacing[1], nx, ny, kind, _lib.SAMPLE_DEVICE_POINTERS, C.byref(o))
    assert rc == _lib.OK, ctx.L.sphx_last_error(ctx.h).decode()
    ctx.synchronize()
    return {k: v.cpu().numpy().astype(np.uint32) if k == "count" else v.cpu().numpy() for k, v in outs.items()}


def check_state(ctx, st, seed, what, kinds=KINDS, torch_too=True):
    """every output on every path, bit for bit against the restatement, and within the float64 bound"""
    K = consts_of(ctx)
    pts = probe_points(st, seed)
    for kind in kinds:
        ref = sr.sample32(K, st, pts, kind)
        dev = ctx.sample(pts, kind)
        assert_bits(dev, ref, "%s kind %d host points" % (what, kind))
        # single fields (the templated subsets) give the same bits
        for f in sr.FIELDS:
            assert_bits(ctx.sample(pts, kind, fields=(f,)), {f: ref[f]}, "%s kind %d %s alone" % (what, kind, f))
        assert_bits(ctx.sample(pts, kind, fields=("density", "velocity")), {k: ref[k] for k in ("density", "velocity")}, what)
        if torch_too:
            import torch

            tp = torch.from_numpy(pts).cuda()
            td = ctx.sample(tp, kind)
            assert_bits({k: v.cpu().numpy().astype(np.uint32) if k == "count" else v.cpu().numpy() for k, v in td.items()}, ref,
                        "%s kind %d device points" % (what, kind))
        g = ctx.sample_grid((F(-0.031), F(-0.047)), (F(0.0227), F(0.0259)), (101, 93), kind)
        gref = sr.sample32(K, st, sr.lattice_points(F(-0.031), F(-0.047), F(0.0227), F(0.0259), 93, 101), kind)
        assert_bits({k: v.reshape(len(gref[k]), -1).squeeze(-1) if k != "velocity" else v.reshape(-1, 2) for k, v in g.items()}, gref,
                    "%s kind %d lattice" % (what, kind))
        if torch_too:  # the lattice through device pointers
            gd = grid_device(ctx, (F(-0.031), F(-0.047)), (F(0.0227), F(0.0259)), (101, 93), kind)
            assert_bits(gd, g, "%s kind %d device lattice" % (what, kind))
        r64, mag, terms = sr.sample64(ctx.params, st, pts, kind)
        sr.assert_within_bound(dev, r64, mag, terms, "%s kind %d" % (what, kind))
        # far and non-finite points: zeros
        tail = slice(len(pts) - 8, len(pts))
        assert not dev["density"][tail].any() and not dev["count"][tail].any() and not dev["fraction"][tail].any()
    return K


def check_solver_consistency(ctx, st, K, kind):
    """at every particle: count = count_dynamic + 1, max(density, rho0) = the solver's density within the bound"""
    counts, _, _ = ctx.download_neighbors()
    assert counts[:, 0].max() < 64
    qi, j, d2 = sr._pairs_within(float(K.h), st["pos"], st["pos"])
    assert d2[qi != j].min() > 1e-10, "a pair closer than 1e-5"
    out = ctx.sample(st["pos"], kind)
    np.testing.assert_array_equal(out["count"], counts[:, 0].astype(np.uint32) + 1)
    r64, mag, terms = sr.sample64(ctx.params, st, st["pos"], kind)
    err = np.abs(np.maximum(out["density"], K.rho0).astype(np.float64) - st["density"].astype(np.float64))
    assert (err <= sr.C * (terms["density"] + sr.K["density"]) * sr.U * mag["density"]).all()
    # the fraction at a particle of the bulk is about one
    assert 0.8 < float(np.median(out["fraction"])) < 1.2


# ----------------------------------------------------------------------------------------------------------------------- state rules
def _rc(ctx, fn="points", kind=0, flags=0, out=None, xy=None, m=4, grid=(0.0, 0.0, 0.1, 0.1, 2, 2)):
    d = np.zeros(8, F)
    o = _lib.SphxSampleOut(density=d.ctypes.data) if out is None else out
    pts = np.zeros((4, 2), F) if xy is None else xy
    if fn == "points":
        return ctx.L.sphx_sample_points(ctx.h, None if pts is False else pts.ctypes.data_as(C.c_void_p), m, kind, flags, C.byref(o) if o else None)
    return ctx.L.sphx_sample_grid(ctx.h, *grid, kind, flags, C.byref(o) if o else None)


def test_state_rules_and_argument_errors():
    ctx = scene_ctx()
    for fn in ("points", "grid"):
        assert _rc(ctx, fn) == _lib.ERR_NOT_READY  # after upload
    assert "sphx_upload" in ctx.L.sphx_last_error(ctx.h).decode()
    ctx.update_neighborhood()
    assert _rc(ctx) == _lib.ERR_NOT_READY and "sphx_update_densities" in ctx.L.sphx_last_error(ctx.h).decode()
    ctx.update_densities(y.KERNEL_WENDLAND_C2)
    assert _rc(ctx) == _lib.OK and _rc(ctx, "grid") == _lib.OK
    ctx.set_boundary(ctx.download_boundary()[0])
    assert _rc(ctx) == _lib.ERR_NOT_READY and "sphx_set_boundary" in ctx.L.sphx_last_error(ctx.h).decode()
    timer = y.TimeManager()
    dfsph_steps(ctx, timer, 2)
    assert _rc(ctx) == _lib.OK
    ctx.step_begin(timer.simulation_step())
    assert _rc(ctx) == _lib.ERR_NOT_READY and _rc(ctx, "grid") == _lib.ERR_NOT_READY
    ctx.step_finish(y.duration_as_secs_f32(timer.update_simulation_step(DIAM, 0.0)))
    assert _rc(ctx) == _lib.OK
    # argument errors, on a ready context
    E = _lib.ERR_INVALID_ARGUMENT
    assert ctx.L.sphx_sample_points(None, None, 0, 0, 0, None) == E
    assert _rc(ctx, out=False) == E                                       # out NULL
    assert _rc(ctx, out=_lib.SphxSampleOut()) == E                        # no output requested
    assert _rc(ctx, "grid", out=_lib.SphxSampleOut()) == E
    assert _rc(ctx, xy=False) == E and "xy" in ctx.L.sphx_last_error(ctx.h).decode()
    assert _rc(ctx, kind=3) == E and _rc(ctx, kind=-1) == E and _rc(ctx, "grid", kind=7) == E
    assert _rc(ctx, flags=2) == E and _rc(ctx, "grid", flags=0x80000000) == E
    for bad in [(0.0, 0.0, 0.0, 0.1, 2, 2), (0.0, 0.0, 0.1, -0.1, 2, 2), (0.0, 0.0, float("nan"), 0.1, 2, 2), (0.0, 0.0, 0.1, float("inf"), 2, 2),
                (float("nan"), 0.0, 0.1, 0.1, 2, 2), (0.0, float("-inf"), 0.1, 0.1, 2, 2), (0.0, 0.0, 0.1, 0.1, 1 << 16, 1 << 15)]:
        assert _rc(ctx, "grid", grid=bad) == E, bad
    assert _rc(ctx, xy=False, m=0) == _lib.OK and _rc(ctx, "grid", grid=(0.0, 0.0, 0.1, 0.1, 0, 5)) == _lib.OK  # no-ops
    # the numpy path takes [m, 2] only
    for bad in (np.zeros((4, 3), F), np.zeros(8, F), np.zeros((2, 2, 2), F)):
        with pytest.raises(ValueError):
            ctx.sample(bad)
    # a step_finish refused for its argument: the step did not finish, a step (or a build + densities) is what is missing
    ctx.step_begin(timer.simulation_step())
    with pytest.raises(y.SphxError):
        ctx.step_finish(-1.0)
    assert _rc(ctx) == _lib.ERR_NOT_READY and "run a step" in ctx.L.sphx_last_error(ctx.h).decode()
    dfsph_steps(ctx, timer, 1)
    assert _rc(ctx) == _lib.OK
    # WCSPH: between its two phases
    w = scene_ctx()
    t = y.TimeManager(cfl_factor=0.2)
    wcsph_steps(w, t, 1)
    assert _rc(w) == _lib.OK
    w.wcsph_step_begin(t.simulation_step())
    assert _rc(w) == _lib.ERR_NOT_READY
    # a tile context is refused
    tc = scene_ctx()
    assert tc.L.sphx_tile_configure(tc.h, 0, 0, 65536, 4, 0, 0) == _lib.OK
    assert _rc(tc) == E and "tile" in tc.L.sphx_last_error(tc.h).decode()


def test_steps_over_zero_fluid_particles():
    """A step over zero fluid particles runs no neighbour build: the boundary's grid may not exist, so a query waits for one."""
    _, bnd = dam_break(1.0)
    pts = np.concatenate([bnd[::37], bnd[::53] + F(0.004)]).astype(F)
    for wcsph in (False, True):
        ctx = y.SphxContext()
        ctx.set_boundary(bnd)
        ctx.upload(np.zeros((0, 2), F))
        t = y.TimeManager(cfl_factor=0.2) if wcsph else y.TimeManager()
        (wcsph_steps if wcsph else dfsph_steps)(ctx, t, 1)
        assert _rc(ctx) == _lib.ERR_NOT_READY and "sphx_update_neighborhood" in ctx.L.sphx_last_error(ctx.h).decode()
        ctx.update_neighborhood()
        ctx.update_densities(y.KERNEL_POLY6)
        st = dict(pos=np.zeros((0, 2), F), vel=np.zeros((0, 2), F), density=np.zeros(0, F), boundary=ctx.download_boundary()[0])
        for kind in KINDS:
            out = ctx.sample(pts, kind)
            assert_bits(out, sr.sample32(consts_of(ctx), st, pts, kind), "zero fluid particles, kind %d" % kind)
            assert (out["density"] > 0).all() and not out["count"].any() and not out["fraction"].any()


# ----------------------------------------------------------------------------------------------------------------------- bit equality
def test_reference_scene_bit_exact_after_1_50_400_steps():
    ctx = scene_ctx()
    timer = y.TimeManager()
    done = 0
    for k in (1, 50, 400):
        dfsph_steps(ctx, timer, k - done)
        done = k
        st = state_of(ctx)
        K = check_state(ctx, st, k, "DFSPH step %d" % k, torch_too=(k != 50))
        check_solver_consistency(ctx, st, K, y.KERNEL_WENDLAND_C2)


def test_wcsph_and_random_scene_bit_exact():
    w = scene_ctx()
    t = y.TimeManager(cfl_factor=0.2)
    wcsph_steps(w, t, 30)
    st = state_of(w)
    K = check_state(w, st, 7, "WCSPH step 30", torch_too=False)
    check_solver_consistency(w, st, K, y.KERNEL_POLY6)
    # a random scene (uniform points in a box, a boundary line under it), after two steps
    pos = (uniform_points(6000, 10000.0, 11) + F(0.3)).astype(F)
    bnd = np.stack([np.arange(0.2, 1.3, 0.005, dtype=F), np.full(len(np.arange(0.2, 1.3, 0.005)), 0.28, F)], -1).astype(F)
    ctx = y.SphxContext()
    ctx.set_boundary(bnd)
    ctx.upload(pos)
    dfsph_steps(ctx, y.TimeManager(), 2)
    check_state(ctx, state_of(ctx), 5, "random scene", torch_too=False)


def test_lattice_equals_points():
    ctx = scene_ctx(2.0)
    dfsph_steps(ctx, y.TimeManager(), 3)
    h, gmin = 0.02, -100.0
    bx = float(np.ceil((0.3 - gmin) / (64 * h)) * 64 * h + gmin)  # the first 64-cell directory block edge right of x = 0.3 (x = 1.12)
    # (the fluid of the scene at scale 2 starts in [0.2, 1.19] x [1.4, 3.39])
    shapes = [((0.2331, 1.4317), (0.0173, 0.0191), (37, 45)),   # odd nx, ny
              ((0.05, 2.0), (0.011, 1.0), (129, 1)),            # one row
              ((0.6, 1.0), (1.0, 0.0097), (1, 211)),            # one column
              ((bx - 0.17, 1.45), (0.0123, 0.0151), (33, 31))]  # across a directory block edge in x (0.17 < 32 * 0.0123)
    for (x0, y0), (dx, dy), (nx, ny) in shapes:
        pts = sr.lattice_points(x0, y0, dx, dy, nx, ny)
        for kind in KINDS:
            g = ctx.sample_grid((F(x0), F(y0)), (F(dx), F(dy)), (ny, nx), kind)
            p = ctx.sample(pts, kind)
            for f in sr.FIELDS:
                a = g[f].reshape(p[f].shape)
                assert np.array_equal(a.view(np.uint32), p[f].view(np.uint32)), (x0, y0, nx, ny, kind, f)
            assert p["count"].any()


def test_float64_bound_at_16M_window_across_the_free_surface():
    ctx = scene_ctx(float(np.sqrt(16e6 / 4050.0)))
    dfsph_steps(ctx, y.TimeManager(), 3)
    d = ctx.download()
    bnd = ctx.download_boundary()[0]
    pos = d["pos"]
    # a 512 x 512 window at 1/3 particle spacing around a point of the free surface (the top of the column, 1/4 in from its left)
    xq = np.quantile(pos[:, 0], 0.25)
    col = pos[np.abs(pos[:, 0] - xq) < 0.05]
    yq = float(col[:, 1].max())
    sp = F(0.0033)
    x0, y0 = F(xq - 256 * sp), F(yq - 256 * sp)
    g = ctx.sample_grid((x0, y0), (sp, sp), (512, 512), y.KERNEL_WENDLAND_C2)
    assert g["fraction"].max() > 0.8 and (g["fraction"] == 0).sum() > 1000  # (the window holds bulk and air)
    pts = sr.lattice_points(x0, y0, sp, sp, 512, 512)
    # host binning: only the particles near the window go into the float64 reference
    near = lambda p: (p[:, 0] > x0 - 0.1) & (p[:, 0] < x0 + 512 * sp + 0.1) & (p[:, 1] > y0 - 0.1) & (p[:, 1] < y0 + 512 * sp + 0.1)
    k = near(pos)
    st = dict(pos=pos[k], vel=d["vel"][k], density=d["density"][k], boundary=bnd[near(bnd)])
    r64, mag, terms = sr.sample64(ctx.params, st, pts, y.KERNEL_WENDLAND_C2)
    flat = {f: g[f].reshape((-1, 2) if f == "velocity" else (-1,)) for f in g}
    sr.assert_within_bound(flat, r64, mag, terms, "16 M window")
    # ... and bit for bit against the float32 restatement (the subset keeps the device order, and holds every particle of the
    # window's cell boxes: the margin, 0.1, exceeds the boxes' reach of two cells, 0.04)
    assert_bits(flat, sr.sample32(consts_of(ctx), st, pts, y.KERNEL_WENDLAND_C2), "16 M window")


# ----------------------------------------------------------------------------------------------------------------------- side effects
def _run(n_steps, query, wcsph=False, run_ahead=True):
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
    pts = probe_points(state_of(ctx), 3)  # (both runs download the state here)
    log = []
    if query:
        import torch

        tp = torch.from_numpy(pts).cuda()
    for _ in range(n_steps):
        if wcsph:
            vmax = ctx.wcsph_step_begin(timer.simulation_step())
            st = ctx.wcsph_step_finish(y.duration_as_secs_f32(timer.update_simulation_step(DIAM, vmax)))
        else:
            vmax = ctx.step_begin(timer.simulation_step(), timer.law(DIAM))
            st = ctx.step_finish(y.duration_as_secs_f32(timer.update_simulation_step(DIAM, vmax)))
        log.append((np.float32(vmax), timer.simulation_step_ns(), st["density_iterations"], st["divergence_iterations"], st["flags"],
                    ctx.last_flags()))
        if query:
            ctx.sample(pts)
            ctx.sample(tp, y.KERNEL_POLY6)
            ctx.sample_grid((F(0.0), F(0.0)), (F(0.05), F(0.05)), (20, 20), y.KERNEL_SPIKY, fields=("count",))
            log[-1] += (ctx.last_flags(),)
    d = ctx.download()
    return log, d


@pytest.mark.parametrize("wcsph, steps, run_ahead", [(False, 100, True), (False, 100, False), (True, 30, True)])
def test_queries_have_no_side_effects(wcsph, steps, run_ahead):
    log_a, a = _run(steps, False, wcsph, run_ahead)
    log_b, b = _run(steps, True, wcsph, run_ahead)
    assert [x[:6] for x in log_b] == log_a and all(x[6] == x[5] for x in log_b)
    for k in ("pos", "vel", "density", "ids"):
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k


# ----------------------------------------------------------------------------------------------------------------------- harness
def test_harness_gauges_match_python():
    steps = 120
    xs = [0.05, 0.2, 0.35, 1.0, 1.9]
    out = subprocess.run([HARNESS, "--scale", "1", "--steps", str(steps), "--warmup", "0", "--gauges", ",".join(map(str, xs))],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    res = json.loads(out.stdout.strip().splitlines()[-1])
    w = y.FluidParticleWorld()
    w.reset_fluid(1.0)
    radius = w.properties()["particle_radius"]
    ctx = y.SphxContext()
    ctx.set_boundary(w.boundary_particles)
    ctx.upload(w.positions)
    timer = y.TimeManager()
    for _ in range(steps):
        timer.on_step_started()
        vmax = ctx.step_begin(timer.simulation_step(), timer.law(DIAM))
        ctx.step_finish(y.duration_as_secs_f32(timer.update_simulation_step(DIAM, vmax)))
    d = ctx.download()
    by_id = np.zeros((len(d["ids"]), 4), np.float32)
    by_id[d["ids"], :2] = d["pos"]
    by_id[d["ids"], 2:] = d["vel"]
    h = 1469598103934665603
    for byte in by_id.tobytes():
        h = ((h ^ byte) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    assert int(res["state_fnv1a"], 16) == h  # the same run
    e = y.gauge_elevation(ctx, xs, 0.0, 2.5 * 1.0, float(radius) / 2.0)
    got = res["gauge_elevations"]
    assert len(got) == len(xs)
    for a, b in zip(got, e):
        assert (a is None and np.isnan(b)) or (a is not None and abs(a - b) <= 1e-9 * abs(b)), (got, e)
    assert any(a is not None and a > 0.1 for a in got)
    # the same rule through the float32 restatement of the column
    ny, ys = sr.gauge_column(0.0, 2.5, float(radius) / 2.0)
    f = ctx.sample_grid((F(xs[1]), F(0.0)), (F(1.0), F(float(radius) / 2.0)), (ny, 1), fields=("fraction",))["fraction"][:, 0]
    assert sr.elevation(ys, f) == e[1] or (np.isnan(e[1]) and np.isnan(sr.elevation(ys, f)))
    # existing invocations print what they printed before; malformed gauge arguments exit with status 2
    plain = subprocess.run([HARNESS, "--scale", "1", "--steps", "2", "--warmup", "0"], capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0 and "gauge" not in plain.stdout
    for bad in (["--gauges", "0.1,x"], ["--gauges", ""], ["--gauges", "0.1,,0.2"], ["--gauges", "0.1", "--gauge-range", "0:1"],
                ["--gauges", "0.1", "--gauge-range", "0:1:0"], ["--gauges", "0.1", "--gauge-range", "1:0:0.1"], ["--gauge-range", "0:1:0.1"],
                ["--gauges", "nan"]):
        r = subprocess.run([HARNESS, "--scale", "1", "--steps", "1", "--warmup", "0"] + bad, capture_output=True, text=True, timeout=120)
        assert r.returncode == 2, bad
    rr = subprocess.run([HARNESS, "--scale", "1", "--steps", "3", "--warmup", "0", "--gauges", "0.2", "--gauge-range", "0:1.5:0.01"],
                        capture_output=True, text=True, timeout=300)
    assert rr.returncode == 0 and len(json.loads(rr.stdout.strip().splitlines()[-1])["gauge_elevations"]) == 1
