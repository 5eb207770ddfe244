"""Free-surface extraction on the device (sphx_surface_contour): every output bit for bit against the numpy restatement of the contract
(tests/contour_reference.py) applied to the device's own downloads (download(), download_boundary(), sample_reference.sample32); the
size edges, the capacity rule, host and device pointers, the state rules and argument errors, no side effects on a run, the Python
polylines and the harness's CSV."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import contour_reference as cr
import sample_reference as sr
import yasph2d_amd as y
from util import dam_break, uniform_points
from yasph2d_amd import _lib

pytestmark = pytest.mark.gpu

F = np.float32
KINDS = (y.KERNEL_WENDLAND_C2, y.KERNEL_POLY6, y.KERNEL_SPIKY)
DIAM = F(0.01)
HARNESS = os.path.join(os.path.dirname(os.path.abspath(y.__file__)), "sphx_harness")
SPRAY_LATTICE = (F(0.27), F(0.27), F(0.0119), F(0.0131), 50, 46)
SENTINEL = 0xDEADBEEF


def dfsph_steps(ctx, timer, k):
    for _ in range(k):
        vmax = ctx.step_begin(timer.simulation_step(), timer.law(DIAM))
        ctx.step_finish(y.duration_as_secs_f32(timer.update_simulation_step(DIAM, vmax)))


def wcsph_steps(ctx, timer, k):
    for _ in range(k):
        vmax = ctx.wcsph_step_begin(timer.simulation_step())
        ctx.wcsph_step_finish(y.duration_as_secs_f32(timer.update_simulation_step(DIAM, vmax)))


def scene_ctx(scale=1.0):
    pos, bnd = dam_break(scale)
    ctx = y.SphxContext()
    ctx.set_boundary(bnd)
    ctx.upload(pos)
    return ctx


def state_of(ctx):
    d = ctx.download()
    assert not ctx.last_flags() & y.FLAG_STRAY_PARTICLES
    return dict(pos=d["pos"], vel=d["vel"], density=d["density"], boundary=ctx.download_boundary()[0])


def consts_of(ctx):
    return sr.Constants(ctx.params, ctx.constants())


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def reference(ctx, st, lattice, iso, kind, field):
    x0, y0, dx, dy, nx, ny = lattice
    values = sr.sample32(consts_of(ctx), st, sr.lattice_points(x0, y0, dx, dy, nx, ny), kind)[field]
    return values, cr.contour32(values, x0, y0, dx, dy, nx, ny, iso)


def device(ctx, lattice, iso, kind, field, **kw):
    x0, y0, dx, dy, nx, ny = lattice
    return ctx.contour((x0, y0), (dx, dy), (ny, nx), iso=iso, field=field, kind=kind, **kw)


def assert_same(dev, values, ref, what):
    if "values" in dev:
        assert np.array_equal(bits(dev["values"]).ravel(), bits(values).ravel()), what + ": lattice values differ"
    assert dev["count"] == ref["count"], "%s: %d segments, the reference has %d" % (what, dev["count"], ref["count"])
    assert np.array_equal(dev["cell"], ref["cell"]), what + ": cells differ"
    a, b = bits(dev["segments"]), bits(ref["segments"])
    assert a.shape == b.shape and np.array_equal(a, b), "%s: %d segments differ" % (what, int((a != b).reshape(len(a), -1).any(1).sum()))


def check(ctx, st, lattice, iso, kind, field, what):
    values, ref = reference(ctx, st, lattice, iso, kind, field)
    dev = device(ctx, lattice, iso, kind, field, values=True)
    assert_same(dev, values, ref, what)
    return values, ref, dev


# ------------------------------------------------------------------------------------------------------------------- spray scene
@pytest.fixture(scope="module")
def spray():
    pos = (uniform_points(700, 2500.0, 11) + F(0.3)).astype(F)
    ctx = y.SphxContext()
    ctx.upload(pos)
    ctx.update_neighborhood()
    ctx.update_densities(y.KERNEL_WENDLAND_C2)
    return ctx, state_of(ctx)


def saddle_counts(ref):
    c, inside = ref["case"], ref["centre_inside"]
    return [int(((c == k) & (inside == w)).sum()) for k in (5, 10) for w in (True, False)]


@pytest.mark.parametrize("iso", [0.5, 0.3])
def test_spray_scene_fraction(spray, iso):
    ctx, st = spray
    for kind in KINDS:
        values, ref, dev = check(ctx, st, SPRAY_LATTICE, iso, kind, "fraction", "spray iso %g kind %d" % (iso, kind))
        lines, closed = cr.lines_of(ref["segments"])
        assert ref["count"] > 300 and all(closed) and cr.dangling(ref["segments"]) == (0, 0)
        if kind == y.KERNEL_WENDLAND_C2:
            # non-vacuity, from the reference: every case, both resolutions of both saddles, closed lines, inside on the left
            print("spray iso %g: %d segments, saddles (5 in, 5 out, 10 in, 10 out) = %s" % (iso, ref["count"], saddle_counts(ref)))
            assert set(np.unique(ref["case"])) == set(range(16))
            assert min(saddle_counts(ref)) >= 3, saddle_counts(ref)
            assert cr.enclosed_area(ref["segments"]) > 0
        # the polylines through the library's stitcher are the reference's
        dl, dc = y.contour_lines(dev["segments"])
        assert dc == [bool(c) for c in closed] and len(dl) == len(lines) and all(np.array_equal(bits(a), bits(b)) for a, b in zip(dl, lines))
    # two calls on one state return the same bytes
    a, b = (device(ctx, SPRAY_LATTICE, iso, y.KERNEL_WENDLAND_C2, "fraction") for _ in range(2))
    assert a["segments"].tobytes() == b["segments"].tobytes() and a["cell"].tobytes() == b["cell"].tobytes()


def test_spray_scene_density(spray):
    ctx, st = spray
    rho0 = float(ctx.params.fluid_density)
    for kind in KINDS:
        for iso in (0.5 * rho0 + 0.37, 0.3 * rho0):
            values, ref, _ = check(ctx, st, SPRAY_LATTICE, F(iso), kind, "density", "spray density iso %g kind %d" % (iso, kind))
            assert ref["count"] > 50 and all(cr.lines_of(ref["segments"])[1])


# ------------------------------------------------------------------------------------------------------------------- dam break
def tank_lattice(st, nx, ny):
    """a lattice over the whole tank: the walls' bounding box and 3 h around it"""
    b = st["boundary"]
    lo, hi = b.min(0) - F(0.06), b.max(0) + F(0.06)
    return (F(lo[0]), F(lo[1]), F((hi[0] - lo[0]) / (nx - 1)), F((hi[1] - lo[1]) / (ny - 1)), nx, ny)


@pytest.fixture(scope="module")
def dam40():
    ctx = scene_ctx()
    dfsph_steps(ctx, y.TimeManager(), 40)
    return ctx, state_of(ctx)


def test_dam_break_dfsph_0_40_150_steps():
    ctx = scene_ctx()
    ctx.update_neighborhood()
    ctx.update_densities(y.KERNEL_WENDLAND_C2)
    timer = y.TimeManager()
    done = 0
    for k in (0, 40, 150):
        dfsph_steps(ctx, timer, k - done)
        done = k
        st = state_of(ctx)
        lat = tank_lattice(st, 131, 97)
        _, ref, _ = check(ctx, st, lat, 0.5, y.KERNEL_WENDLAND_C2, "fraction", "DFSPH step %d fraction" % k)
        # the fluid lies inside the tank: its surface closes and encloses about the fluid's area (4050 particles / 10000 per m^2);
        # a region of 0.2 m^2 has a perimeter of 2 sqrt(0.2 pi) = 1.6 m at least, i.e. 50 segments no longer than a cell's diagonal
        lines, closed = cr.lines_of(ref["segments"])
        assert all(closed) and cr.enclosed_area(ref["segments"]) > 0.2 and ref["count"] > 50
        # the density counts the walls: its contour runs along them and ends on the lattice border or closes
        check(ctx, st, lat, 0.5 * float(ctx.params.fluid_density), y.KERNEL_WENDLAND_C2, "density", "DFSPH step %d density" % k)


def test_dam_break_wcsph_20_steps():
    ctx = scene_ctx()
    wcsph_steps(ctx, y.TimeManager(cfl_factor=0.2), 20)
    st = state_of(ctx)
    lat = tank_lattice(st, 131, 97)
    for kind in (y.KERNEL_POLY6, y.KERNEL_SPIKY):
        _, ref, _ = check(ctx, st, lat, 0.5, kind, "fraction", "WCSPH step 20 kind %d" % kind)
        assert ref["count"] > 50
    check(ctx, st, lat, 0.5 * float(ctx.params.fluid_density), y.KERNEL_POLY6, "density", "WCSPH step 20 density")


# ------------------------------------------------------------------------------------------------------------------- size edges
def test_size_edges(dam40):
    ctx, st = dam40
    x, top = (float(v) for v in st["pos"][np.argsort(st["pos"][:, 1])[-50]])  # a particle just under the free surface
    for nx, ny in ((2, 2), (2, 37), (41, 2), (18, 16), (66, 5), (258, 3), (1, 5), (7, 1), (1, 1)):  # 255, 260 and 514 cells among them
        lat = (F(x - 0.004 * nx), F(top - 0.004 * ny), F(0.0083), F(0.0079), nx, ny)
        values, ref, dev = check(ctx, st, lat, 0.5, y.KERNEL_WENDLAND_C2, "fraction", "lattice %d x %d" % (nx, ny))
        if (nx, ny) in ((18, 16), (2, 37)):  # (across the surface: bulk below, air above)
            assert ref["count"] > 0 and values.any(), (nx, ny)
    assert device(ctx, (F(0), F(0), F(0.1), F(0.1), 0, 7), 0.5, 0, "fraction", values=True)["count"] == 0
    # wholly in air, wholly in bulk
    air = (F(1.5), F(1.2), F(0.004), F(0.004), 40, 30)
    values, ref, dev = check(ctx, st, air, 0.5, y.KERNEL_WENDLAND_C2, "fraction", "air")
    assert dev["count"] == 0 and not values.any()
    lo = st["pos"].min(0)
    bulk = (F(lo[0] + 0.05), F(lo[1] + 0.05), F(0.004), F(0.004), 30, 30)
    values, ref, dev = check(ctx, st, bulk, 0.5, y.KERNEL_WENDLAND_C2, "fraction", "bulk")
    assert dev["count"] == 0 and (values >= F(0.5)).all() and (ref["case"] == 15).all()


def test_large_lattice_carries_across_workgroups(dam40):
    ctx, st = dam40
    nx, ny = 1025, 513
    lat = tank_lattice(st, nx, ny)
    x0, y0, dx, dy = lat[:4]
    dev = device(ctx, lat, 0.5, y.KERNEL_WENDLAND_C2, "fraction", values=True)
    # the values are sphx_sample_grid's bits, and (on every 8th row and column) the restatement's
    g = ctx.sample_grid((x0, y0), (dx, dy), (ny, nx), y.KERNEL_WENDLAND_C2, fields=("fraction",))["fraction"]
    assert np.array_equal(bits(dev["values"]), bits(g))
    pts = sr.lattice_points(x0, y0, dx, dy, nx, ny).reshape(ny, nx, 2)[::8, ::8].reshape(-1, 2)
    sub = sr.sample32(consts_of(ctx), st, pts, y.KERNEL_WENDLAND_C2)["fraction"]
    assert np.array_equal(bits(sub), bits(g[::8, ::8]).ravel())
    ref = cr.contour32(g, x0, y0, dx, dy, nx, ny, 0.5)
    assert_same(dev, g, ref, "1025 x 513")
    # segments in many workgroups of 256 cells (a lattice row is four of them, the surface crosses many rows), further apart than
    # the 256 totals the carry pass scans at a time: the carry crossed workgroups and chunks
    blocks = np.unique(ref["cell"] // 256)
    print("1025 x 513: %d segments in %d workgroups, %d apart" % (ref["count"], len(blocks), blocks.max() - blocks.min()))
    assert ref["count"] > 256 and len(blocks) > 100 and blocks.max() - blocks.min() > 256
    assert (np.diff(dev["cell"].astype(np.int64)) >= 0).all()


# ------------------------------------------------------------------------------------------------------------------- output variants
def raw_call(ctx, lattice, iso, cap, seg, cell, values, count, flags=0, kind=0, field=0):
    x0, y0, dx, dy, nx, ny = lattice
    ptr = (lambda a: None if a is None else a.ctypes.data) if flags == 0 else (lambda t: None if t is None else t.data_ptr())
    o = _lib.SphxContourOut(segments=ptr(seg), cell=ptr(cell), values=ptr(values), count=ptr(count))
    return ctx.L.sphx_surface_contour(ctx.h, x0, y0, dx, dy, nx, ny, kind, field, iso, cap, flags, C.byref(o))


def test_capacity_and_count_only(spray):
    ctx, st = spray
    _, ref = reference(ctx, st, SPRAY_LATTICE, 0.5, 0, "fraction")
    n = ref["count"]
    for cap in (0, 1, n // 2, n - 1, n, n + 5):
        seg, cell, cnt = np.full((n + 8, 4), SENTINEL, np.uint32), np.full(n + 8, SENTINEL, np.uint32), np.zeros(1, np.uint32)
        assert raw_call(ctx, SPRAY_LATTICE, 0.5, cap, seg, cell, None, cnt) == _lib.OK
        k = min(cap, n)
        assert cnt[0] == n
        assert np.array_equal(seg[:k], bits(ref["segments"]).reshape(-1, 4)[:k]) and np.array_equal(cell[:k], ref["cell"][:k])
        assert (seg[k:] == SENTINEL).all() and (cell[k:] == SENTINEL).all(), "memory behind the capacity was written (cap %d)" % cap
    cnt = np.zeros(1, np.uint32)
    assert raw_call(ctx, SPRAY_LATTICE, 0.5, 1 << 30, None, None, None, cnt) == _lib.OK and cnt[0] == n  # segments NULL: the count alone
    cell = np.full(n, SENTINEL, np.uint32)
    assert raw_call(ctx, SPRAY_LATTICE, 0.5, n, None, cell, None, cnt) == _lib.OK and np.array_equal(cell, ref["cell"])  # cells alone
    # the Python call: a too small guess is repeated with the exact count; an explicit cap is kept
    assert device(ctx, SPRAY_LATTICE, 0.5, 0, "fraction", cap=10)["segments"].shape == (10, 2, 2)
    assert device(ctx, SPRAY_LATTICE, 0.5, 0, "fraction", cap=0)["count"] == n
    fine = (SPRAY_LATTICE[0], SPRAY_LATTICE[1], F(0.0017), F(0.0019), 340, 310)  # more segments than the first guess holds
    d = device(ctx, fine, 0.3, 0, "fraction")
    assert d["count"] > 8 * (340 + 310) and len(d["segments"]) == d["count"]
    assert_same(d, None, reference(ctx, st, fine, 0.3, 0, "fraction")[1], "fine lattice")


def test_device_pointers_agree_with_the_host_path(spray):
    import torch

    ctx, st = spray
    x0, y0, dx, dy, nx, ny = SPRAY_LATTICE
    for field, iso in (("fraction", 0.5), ("density", 37.5)):
        host = device(ctx, SPRAY_LATTICE, iso, y.KERNEL_POLY6, field, values=True)
        n = host["count"]
        for cap in (n + 7, n // 3):
            out = dict(segments=torch.full((cap + 4, 2, 2), -7.0, device="cuda"), cell=torch.full((cap + 4,), -7, dtype=torch.int32, device="cuda"),
                       values=torch.full((ny, nx), -7.0, device="cuda"), count=torch.full((1,), -7, dtype=torch.int32, device="cuda"))
            d = ctx.contour((x0, y0), (dx, dy), (ny, nx), iso=iso, field=field, kind=y.KERNEL_POLY6, cap=cap, out=out)
            k = min(cap, n)
            assert d["count"] == n and np.array_equal(bits(d["values"].cpu().numpy()), bits(host["values"]))
            assert np.array_equal(bits(d["segments"].cpu().numpy()), bits(host["segments"][:k]))
            assert np.array_equal(d["cell"].cpu().numpy().astype(np.uint32), host["cell"][:k])
            assert (out["segments"][k:] == -7).all() and (out["cell"][k:] == -7).all()  # nothing behind min(count, cap)
        # the count alone, and the values into the caller's tensor
        only = dict(values=torch.full((ny, nx), -7.0, device="cuda"))
        d = ctx.contour((x0, y0), (dx, dy), (ny, nx), iso=iso, field=field, kind=y.KERNEL_POLY6, out=only)
        assert d["count"] == n and np.array_equal(bits(d["values"].cpu().numpy()), bits(host["values"]))
    # values are sphx_sample_grid's bits
    for kind in KINDS:
        g = ctx.sample_grid((x0, y0), (dx, dy), (ny, nx), kind, fields=("fraction", "density"))
        for field in ("fraction", "density"):
            assert np.array_equal(bits(device(ctx, SPRAY_LATTICE, 0.5, kind, field, values=True)["values"]), bits(g[field]))


# ------------------------------------------------------------------------------------------------------------------- rules
def _rc(ctx, lattice=(0.0, 0.0, 0.1, 0.1, 3, 3), iso=0.5, cap=8, flags=0, kind=0, field=0, out=True, count=True):
    seg, cnt = np.zeros((8, 4), F), np.full(1, 77, np.uint32)
    x0, y0, dx, dy, nx, ny = lattice
    o = _lib.SphxContourOut(segments=seg.ctypes.data, count=cnt.ctypes.data if count else None)
    rc = ctx.L.sphx_surface_contour(ctx.h, x0, y0, dx, dy, nx, ny, kind, field, iso, cap, flags, C.byref(o) if out else None)
    return rc, int(cnt[0])


def test_state_rules_and_argument_errors():
    OK, E, NR = _lib.OK, _lib.ERR_INVALID_ARGUMENT, _lib.ERR_NOT_READY
    ctx = scene_ctx()
    err = lambda: ctx.L.sphx_last_error(ctx.h).decode()
    assert _rc(ctx)[0] == NR and "sphx_upload" in err()
    ctx.update_neighborhood()
    assert _rc(ctx)[0] == NR and "sphx_update_densities" in err()
    ctx.update_densities(y.KERNEL_WENDLAND_C2)
    assert _rc(ctx)[0] == OK
    ctx.set_boundary(ctx.download_boundary()[0])
    assert _rc(ctx)[0] == NR and "sphx_set_boundary" in err()
    timer = y.TimeManager()
    dfsph_steps(ctx, timer, 2)
    assert _rc(ctx)[0] == OK
    ctx.step_begin(timer.simulation_step())
    assert _rc(ctx)[0] == NR
    assert _rc(ctx, lattice=(0.0, 0.0, 0.1, 0.1, 0, 5)) == (OK, 0)  # an empty lattice: a no-op once the arguments pass, as sphx_sample_grid
    ctx.step_finish(y.duration_as_secs_f32(timer.update_simulation_step(DIAM, 0.0)))
    assert _rc(ctx)[0] == OK
    w = scene_ctx()
    t = y.TimeManager(cfl_factor=0.2)
    wcsph_steps(w, t, 1)
    assert _rc(w)[0] == OK
    w.wcsph_step_begin(t.simulation_step())
    assert _rc(w)[0] == NR
    # argument errors, on a ready context
    assert ctx.L.sphx_surface_contour(None, 0.0, 0.0, 0.1, 0.1, 2, 2, 0, 0, 0.5, 0, 0, None) == E
    assert _rc(ctx, out=False)[0] == E and "out" in err()
    assert _rc(ctx, count=False)[0] == E and "count" in err()
    for iso in (float("nan"), float("inf"), float("-inf")):
        assert _rc(ctx, iso=iso)[0] == E and "iso" in err()
    assert _rc(ctx, field=2)[0] == E and "field" in err() and _rc(ctx, field=-1)[0] == E
    assert _rc(ctx, flags=2)[0] == E and "flags" in err() and _rc(ctx, flags=0x80000000)[0] == E
    assert _rc(ctx, kind=3)[0] == E and _rc(ctx, kind=-1)[0] == E
    for bad in [(0.0, 0.0, 0.0, 0.1, 2, 2), (0.0, 0.0, 0.1, -0.1, 2, 2), (0.0, 0.0, float("nan"), 0.1, 2, 2), (0.0, 0.0, 0.1, float("inf"), 2, 2),
                (float("nan"), 0.0, 0.1, 0.1, 2, 2), (0.0, float("-inf"), 0.1, 0.1, 2, 2), (0.0, 0.0, 0.1, 0.1, 1 << 16, 1 << 15)]:
        assert _rc(ctx, lattice=bad)[0] == E, bad
    # count = 0 without a cell
    for lat in ((0.0, 0.0, 0.1, 0.1, 1, 9), (0.0, 0.0, 0.1, 0.1, 9, 1), (0.0, 0.0, 0.1, 0.1, 0, 0)):
        assert _rc(ctx, lattice=lat) == (OK, 0), lat
    with pytest.raises(ValueError):
        ctx.contour((0, 0), 0.1, (3, 3), field="velocity")
    # a tile context is refused
    tc = scene_ctx()
    assert tc.L.sphx_tile_configure(tc.h, 0, 0, 65536, 4, 0, 0) == OK
    assert _rc(tc)[0] == E and "tile" in tc.L.sphx_last_error(tc.h).decode()


def test_contour_calls_have_no_side_effects():
    import torch

    def run(query):
        ctx = scene_ctx()
        timer = y.TimeManager()
        lat = (F(-0.05), F(-0.05), F(0.021), F(0.019), 110, 90)
        out = dict(segments=torch.zeros((4096, 4), device="cuda"), cell=torch.zeros(4096, dtype=torch.int32, device="cuda"))
        for _ in range(20):
            dfsph_steps(ctx, timer, 1)
            if query:
                assert device(ctx, lat, 0.5, y.KERNEL_WENDLAND_C2, "fraction", values=True)["count"] > 0
                device(ctx, lat, 50.0, y.KERNEL_POLY6, "density")
                ctx.contour(lat[:2], lat[2:4], (lat[5], lat[4]), kind=y.KERNEL_SPIKY, out=out)
        return ctx.state_digest(), timer.simulation_step_ns(), ctx.last_flags()

    assert run(True) == run(False)


# ------------------------------------------------------------------------------------------------------------------- harness
def test_harness_contour_out_matches_python(tmp_path):
    steps = 40
    grid = (-0.05, -0.05, 0.0173, 0.0191, 128, 90)
    path = tmp_path / "contour.csv"
    out = subprocess.run([HARNESS, "--scale", "1", "--steps", str(steps), "--warmup", "0", "--contour-out", str(path), "--contour-grid",
                          ",".join(map(str, grid)), "--contour-iso", "0.45"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    w = y.FluidParticleWorld()
    w.reset_fluid(1.0)
    ctx = y.SphxContext()
    ctx.set_boundary(w.boundary_particles)
    ctx.upload(w.positions)
    timer = y.TimeManager()
    for _ in range(steps):
        timer.on_step_started()
        vmax = ctx.step_begin(timer.simulation_step(), timer.law(DIAM))
        ctx.step_finish(y.duration_as_secs_f32(timer.update_simulation_step(DIAM, vmax)))
    d = ctx.contour((F(grid[0]), F(grid[1])), (F(grid[2]), F(grid[3])), (grid[5], grid[4]), iso=F(0.45))
    lines, closed = y.contour_lines(d["segments"])
    rows = open(path).read().splitlines()
    assert rows[0] == "line,closed,x,y" and len(rows) - 1 == sum(len(l) for l in lines) > 100
    got = np.array([[float(v) for v in r.split(",")] for r in rows[1:]])
    want = np.concatenate([np.concatenate([np.full((len(l), 1), k), np.full((len(l), 1), int(c)), l.astype(np.float64)], 1)
                           for k, (l, c) in enumerate(zip(lines, closed))])
    assert np.array_equal(got[:, :2], want[:, :2]) and np.array_equal(got[:, 2:].astype(F), want[:, 2:].astype(F))
    assert '"contour_segments": %d' % d["count"] in out.stdout and '"contour_lines": %d' % len(lines) in out.stdout
    # existing invocations print what they printed before; malformed arguments exit with status 2
    plain = subprocess.run([HARNESS, "--scale", "1", "--steps", "2", "--warmup", "0"], capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0 and "contour" not in plain.stdout
    for bad in (["--contour-grid", "0,0,0.1,0.1,4,4"], ["--contour-iso", "0.5"], ["--contour-out", str(path), "--contour-grid", "0,0,0.1,0.1,4"],
                ["--contour-out", str(path), "--contour-grid", "0,0,0,0.1,4,4"], ["--contour-out", str(path), "--contour-iso", "nan"],
                ["--contour-out", str(path), "--contour-grid", "0,0,0.1,0.1,4.5,4"], ["--contour-out", ""]):
        r = subprocess.run([HARNESS, "--scale", "1", "--steps", "1", "--warmup", "0"] + bad, capture_output=True, text=True, timeout=120)
        assert r.returncode == 2, bad
    # the default lattice covers the scene
    r = subprocess.run([HARNESS, "--scale", "1", "--steps", "1", "--warmup", "0", "--contour-out", str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and '"contour_segments"' in r.stdout and len(open(path).read().splitlines()) > 100
