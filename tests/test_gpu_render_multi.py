"""The picture of a tiled run on the device (include/sphx.h, "picture of a tiled run"): sphx_multi_render, sphx_multi_render_layer and
sphx_tile_render_layer against tests/render_multi_reference.py, bit for bit.  The truth is always computed from what the tiles' own
sphx_download returns (owned = bit 31 of the id) and each tile's sphx_download_boundary: layer32 per tile, merged by the composite rule.
All scenes are the dam break of tests/util.py at scale 1.0 (4 050 particles, every tile on device 0), all images at most 320 x 240.
The exports, sphx_render_merge, the window header under hostile values and the rule itself on the golden states are checked without
a GPU in tests/test_render_multi_host.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import render_multi_reference as rm
import render_reference as rr
import yasph2d_amd as y
from tiles_reference import GridLayout, StripLayout, cell_coord, quantile_cuts
from util import dam_break
from yasph2d_amd import _lib
from yasph2d_amd.multi import MultiSolver

pytestmark = pytest.mark.gpu

F = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
POS, BOUNDARY = dam_break(1.0)
N = len(POS)
NONE, BND = rm.NONE, rm.BOUNDARY
H = rm.SMOOTHING_LENGTH
STEP_FIELDS = tuple(k for k, _ in _lib.SphxStepStats._fields_)


def refused(code, fn, *args, **kw):
    with pytest.raises(y.SphxError) as e:
        fn(*args, **kw)
    assert e.value.code == code, str(e.value)
    return str(e.value)


def make_multi(world, params=None, rebalance_every=4, halo=10, strips=None, grid=None, invariant=False, pos=POS, boundary=BOUNDARY):
    m = MultiSolver(params if params is not None else y.default_params(), devices=[0] * world, halo=halo, rebalance_every=rebalance_every)
    if invariant:
        m.set_tiling_invariant(True)
    if strips is not None:
        m.set_strips(*strips)
    if grid is not None:
        m.set_grid(*grid)
    m.set_boundary(boundary)
    m.upload(pos)
    return m


def tile_states(m, world):
    """[(download, boundary)] of every tile: the inputs of the reference"""
    out = []
    for k in range(world):
        t = m.tile_context(k)
        out.append((t.download(), t.download_boundary()[0]))
    return out


def same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("key", "owner", "rgba"))


def check_view(m, tiles, view, what, rects=None):
    """sphx_multi_render (rgba, owner ids) and sphx_multi_render_layer (key, owner, rgba) against merge(layer32 per tile); returns the
    reference layers and their merge"""
    layers = [rm.layer32(t, b, view, rect=None if rects is None else rects[k]) for k, (t, b) in enumerate(tiles)]
    want = rm.merge(layers)
    img, own = m.render(owner=True, **view.fields())
    assert np.array_equal(own, want["owner"]), what + ": owners"
    assert np.array_equal(img, want["rgba"]), what + ": rgba"
    got = m.render_layer(**view.fields())
    assert same(got, want), what + ": layer"
    assert np.array_equal(m.render(**view.fields()), want["rgba"]) and np.array_equal(m.render(owner=True, rgba=False, **view.fields()), want["owner"]), what
    return layers, want


def seam_point(tiles):
    """the midpoint of the closest pair of owned particles of tile 0 and the first tile of the next column (2 strips: tile 1; 2 x 2, rank
    = ix * ny + iy: tile 2): a point on a cut along x, inside the fluid"""
    other = 1 if len(tiles) == 2 else 2
    a = tiles[0][0]["pos"][(tiles[0][0]["ids"] >> 31) == 1].astype(np.float64)
    b = tiles[other][0]["pos"][(tiles[other][0]["ids"] >> 31) == 1].astype(np.float64)
    d = ((a[:, None, :] - b[None, :, :]) ** 2).sum(axis=2)
    i, j = np.unravel_index(d.argmin(), d.shape)
    return tuple(float(v) for v in (a[i] + b[j]) * 0.5)


def views_of(tiles, world):
    d = np.concatenate([t["pos"][(t["ids"] >> 31) == 1] for t, _ in tiles])
    c = seam_point(tiles) if world > 1 else (float(np.median(d[:, 0])), float(np.median(d[:, 1])))
    edge = (float(d[:, 0].max()), float(d[:, 1].max()))  # the fluid's upper right corner: three quarters of the view are outside it
    return [("whole scene, radius 0.015", rr.fit(320, 240, radius=0.015), True),
            ("reference radius", rr.fit(320, 240), False),
            ("zoom onto a cut, radius h", rr.View(160, 120, c, 2000.0, radius=H), True),
            ("37 x 23 on a cut", rr.View(37, 23, c, 400.0, radius=0.01), False),
            ("half outside the fluid", rr.View(160, 120, edge, 300.0, radius=0.015), False),
            ("zoomed out, min_pixel_radius 0.75", rr.fit(160, 120, (-1.0, -1.0, 6.0, 5.0), min_pixel_radius=0.75), False)]


# ---- 1. default mode -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [1, 2, 4], ids=["one tile", "2 strips", "2x2"])
def test_default_mode_against_the_reference(world):
    # (2 strips: cut along x, as the golden states of the host test are — across a cut along y the tile with the greater y nearly always
    # holds the greater Morton code, and "last wins" would pass; cut at the first third of the particles, so that the loads differ and
    # the run re-partitions)
    m = make_multi(world, strips=(0, [0, quantile_cuts(cell_coord(POS, 0), 3)[1], 65536]) if world == 2 else None)
    for state in ("after the upload", "after 40 steps"):
        if state == "after 40 steps":
            m.steps(y.TimeManager(), 40)
            if world > 1:
                assert m.info()["rebalances"] >= 1, m.info()
        tiles = tile_states(m, world)
        assert sum(int(((t["ids"] >> 31) == 1).sum()) for t, _ in tiles) == N
        for name, view, seam in views_of(tiles, world):
            what = "%d tiles, %s, %s" % (world, state, name)
            layers, want = check_view(m, tiles, view, what)
            fluid = want["owner"] < BND
            assert fluid.any(), what
            if "cut" not in name:  # (the two zooms onto a cut are inside the fluid)
                assert (want["owner"] == NONE).any(), what
            if world > 1 and seam:  # the seams are under load: either naive merge order would fail
                multi, not_lowest, not_highest = rm.seam_counts(layers)
                print("%s: %d pixels covered by two or more tiles, winner not the lowest rank at %d, not the highest at %d" % (what, multi, not_lowest, not_highest))
                assert multi >= 100 and not_lowest >= 20 and not_highest >= 20, what
        if world == 1:  # one tile: sphx_render's picture of that particle set, ids for indices
            t, b = tiles[0]
            view = rr.fit(320, 240, radius=0.015)
            single = rr.render32(dict(pos=t["pos"], vel=t["vel"], boundary=b), view, rm.PARTICLE_RADIUS)
            img, own = m.render(owner=True, **view.fields())
            fl = single["owner"] < BND
            assert np.array_equal(img, single["rgba"]) and np.array_equal(own[~fl], single["owner"][~fl])
            assert np.array_equal(own[fl], t["ids"][single["owner"][fl]] & 0x7FFFFFFF)
    m.close()


# ---- 2. one tile -------------------------------------------------------------------------------------------------------------------------------
def explicit(world):
    cx, cy = cell_coord(POS, 0), cell_coord(POS, 1)
    if world == 2:
        lay = StripLayout(1, quantile_cuts(cy, 2))
        return dict(strips=(1, lay.cuts)), lay.rects()
    lay = GridLayout.quantile(POS, 2, 2)
    return dict(grid=(lay.xcuts, lay.ycuts)), lay.rects()


@pytest.mark.parametrize("world", [2, 4], ids=["2 strips", "2x2"])
def test_per_tile_layers_host_and_device_pointers(world):
    """sphx_tile_render_layer of tile k = layer32 of tile k (its owned particles, the boundary particles of its cells), through host
    pointers and through device pointers; explicit cuts, no re-partitioning: the rectangles are known"""
    import torch

    kw, rects = explicit(world)
    m = make_multi(world, rebalance_every=0, **kw)
    m.steps(y.TimeManager(), 10)
    tiles = tile_states(m, world)
    for name, view, _ in views_of(tiles, world)[:4]:
        layers, want = check_view(m, tiles, view, "%d tiles, %s" % (world, name), rects=rects)
        for k in range(world):
            tc = m.tile_context(k)
            what = "%d tiles, %s, tile %d" % (world, name, k)
            got = tc.tile_render_layer(**view.fields())
            assert same(got, layers[k]), what
            dev = tc.tile_render_layer(device=True, **view.fields())
            torch.cuda.synchronize()
            for f, dt in (("key", np.uint32), ("owner", np.uint32), ("rgba", np.uint8)):
                assert np.array_equal(dev[f].cpu().numpy().view(dt).reshape(layers[k][f].shape), layers[k][f]), what + ": device pointers, " + f
            assert "tile" in refused(_lib.ERR_INVALID_ARGUMENT, tc.render, **view.fields())  # sphx_render keeps refusing a tile context
        # the layers of the tiles, merged by sphx_render_merge, are the multi's layer
        assert same(y.render_merge([m.tile_context(k).tile_render_layer(**view.fields()) for k in range(world)]), want)
    plain = y.SphxContext()
    plain.set_boundary(BOUNDARY)
    plain.upload(POS)
    assert "not a tile context" in refused(_lib.ERR_INVALID_ARGUMENT, plain.tile_render_layer, width=32, height=16)
    win, lay = (C.c_uint32 * 4)(), _lib.SphxRenderLayer()
    assert plain.L.sphx_tile_render_window(plain.h, C.byref(y.render_fit(32, 16)), 1, win, C.byref(lay)) == _lib.ERR_INVALID_ARGUMENT
    plain.close()
    m.close()


# ---- 3. every tiling draws the same picture ----------------------------------------------------------------------------------------------------
def test_tiling_invariant_mode_equals_the_single_context():
    """30 steps as a single context, as 2 strips and as 2 x 2 in tiling-invariant mode (fixed 2 + 2 iterations): the same particle set bit
    for bit, so the tiled pictures are the single context's render with ids[owner] substituted"""
    steps = 30
    params = y.default_params(fixed_iterations=(2, 2))
    ctx = y.SphxContext(params)
    ctx.set_tiling_invariant(True)
    ctx.set_boundary(BOUNDARY)
    ctx.upload(POS)
    timer = y.TimeManager()
    for _ in range(steps):
        vmax = ctx.step_begin(timer.simulation_step(), timer.law(F(0.01)))
        ctx.step_finish(y.duration_as_secs_f32(timer.update_simulation_step(F(0.01), vmax)))
    d = ctx.download()
    ids = d["ids"]
    mid = (float(np.median(d["pos"][:, 0])), float(np.median(d["pos"][:, 1])))  # (the tiles' cuts sit at the particle-count quantiles)
    views = [rr.fit(320, 240, radius=0.015), rr.fit(320, 240), rr.View(160, 120, mid, 1500.0, radius=H)]
    single = []
    for v in views:
        img, own = ctx.render(owner=True, **v.fields())
        fl = own < BND
        assert fl.any()
        single.append((img, np.where(fl, ids[np.where(fl, own, 0)], own).astype(np.uint32)))
    for world in (2, 4):
        m = make_multi(world, params=y.default_params(fixed_iterations=(2, 2)), invariant=True)
        t2 = y.TimeManager()
        m.steps(t2, steps)
        assert t2.simulation_step_ns() == timer.simulation_step_ns()
        for v, (img, own) in zip(views, single):
            gi, go = m.render(owner=True, **v.fields())
            assert np.array_equal(go, own) and np.array_equal(gi, img), world
        m.close()
    ctx.close()


# ---- 4. extremes -----------------------------------------------------------------------------------------------------------------------------------
def test_extremes_empty_tile_walls_only_and_particles_beyond_the_domain():
    # a tile that owns nothing: three strips along x, the third to the right of the fluid (cells >= 5100: x >= 2.0)
    cuts = [0, 5017, 5100, 65536]
    m = make_multi(3, rebalance_every=0, strips=(0, cuts))
    m.steps(y.TimeManager(), 5)
    tiles = tile_states(m, 3)
    assert ((tiles[2][0]["ids"] >> 31) == 0).all()
    rects = StripLayout(0, cuts).rects()
    for view in (rr.fit(320, 240, radius=0.015), rr.View(160, 120, (0.34, 1.0), 800.0, radius=H)):
        layers, want = check_view(m, tiles, view, "3 strips, one empty", rects=rects)
        got = m.tile_context(2).tile_render_layer(**view.fields())
        assert same(got, layers[2]) and not (got["owner"] < BND).any() and (got["key"] == 0).all()
    # walls only: the lower right corner of the box, far from the fluid
    view = rr.View(120, 90, (2.0, 0.0), 400.0)
    layers, want = check_view(m, tiles, view, "walls only", rects=rects)
    assert (want["owner"] == BND).any() and (want["owner"] == NONE).any() and not (want["owner"] < BND).any()
    m.close()
    # particles pushed beyond the domain (x < grid_min = -100: the saturated cell column 0, owned by the tile whose rectangle starts
    # at 0) are drawn when the view looks there
    out = np.array([[-100.3, 0.8], [-100.31, 0.95], [-100.29, 1.1], [-100.3, 1.25]], F)
    pos = np.concatenate([POS, out])
    m = make_multi(2, rebalance_every=0, strips=(0, [0, 5017, 65536]), pos=pos)
    tiles = tile_states(m, 2)
    own0 = tiles[0][0]["ids"][(tiles[0][0]["ids"] >> 31) == 1] & 0x7FFFFFFF
    assert set(range(N, N + 4)) <= set(own0.tolist())
    view = rr.View(64, 48, (-100.3, 1.0), 80.0, radius=H)
    layers, want = check_view(m, tiles, view, "beyond the domain")
    assert set(np.unique(want["owner"][want["owner"] < BND]).tolist()) == set(range(N, N + 4))
    check_view(m, tiles, rr.fit(320, 240, radius=0.015), "beyond the domain, whole scene")
    m.close()


# ---- 5. no side effects ----------------------------------------------------------------------------------------------------------------------------
def test_a_run_with_renders_is_bit_identical_to_the_run_without():
    steps = 40
    views = [rr.fit(320, 240, radius=0.015), rr.View(160, 120, (0.35, 0.8), 1000.0, radius=H)]

    def run(observed):
        m = make_multi(4)
        timer = y.TimeManager()
        out = []
        for k in range(steps):
            out.append(m.step(timer))
            if observed:
                m.render(owner=True, **views[k % 2].fields())
                m.render_layer(**views[(k + 1) % 2].fields())
                if k % 5 == 0:
                    m.tile_context(k % 4).tile_render_layer(**views[0].fields())
        d, info = m.download(), m.info()
        m.close()
        return d, out, info

    da, sa, ia = run(False)
    db, sb, ib = run(True)
    for k in ("ids", "pos", "vel", "density"):
        assert da[k].tobytes() == db[k].tobytes(), k
    for k, (a, b) in enumerate(zip(sa, sb)):
        for f in STEP_FIELDS + ("dt_ns",):
            assert np.array(a[f]).tobytes() == np.array(b[f]).tobytes(), (k, f, a[f], b[f])
    assert len(STEP_FIELDS) == 12 and set(STEP_FIELDS) <= set(sa[0])
    assert ia["exchanges"] == ib["exchanges"] and ia["rebalances"] == ib["rebalances"] >= 1 and ia["halo_now"] == ib["halo_now"]


# ---- 6. state rules and argument errors ------------------------------------------------------------------------------------------------------------
def test_state_rules_and_argument_errors():
    E, OK, NR = _lib.ERR_INVALID_ARGUMENT, _lib.OK, _lib.ERR_NOT_READY
    m = MultiSolver(y.default_params(), devices=[0, 0], halo=10, rebalance_every=4)
    L, h = m.L, m.h
    buf = np.zeros((3, 32 * 16), np.uint32)

    def call(layer, view=None, flags=0, out=None, **fields):
        v = y.render_fit(32, 16)
        for k, val in fields.items():
            if k == "center":
                v.center[0], v.center[1] = val
            else:
                setattr(v, k, val)
        if layer:
            o = _lib.SphxRenderLayer(buf[0].ctypes.data, buf[1].ctypes.data, buf[2].ctypes.data) if out is None else out
            rc = L.sphx_multi_render_layer(h, None if view is False else C.byref(v), flags, None if o is False else C.byref(o))
        else:
            o = _lib.SphxRenderOut(rgba=buf[2].ctypes.data, owner=buf[1].ctypes.data) if out is None else out
            rc = L.sphx_multi_render(h, None if view is False else C.byref(v), flags, None if o is False else C.byref(o))
        return rc, L.sphx_multi_last_error(h).decode()

    # before the first upload
    for layer in (False, True):
        rc, msg = call(layer)
        assert rc == NR and "sphx_multi_upload" in msg, msg
    m.set_boundary(BOUNDARY)
    m.upload(POS)
    hh = float(H)
    for layer in (False, True):
        fn = "sphx_multi_render_layer" if layer else "sphx_multi_render"
        assert call(layer)[0] == OK
        nothing = _lib.SphxRenderLayer() if layer else _lib.SphxRenderOut()
        for kw, word in [(dict(view=False), "view"), (dict(out=False), "out"), (dict(out=nothing), "no output"), (dict(flags=1), "flags"), (dict(flags=2), "flags"),
                         (dict(flags=0x80000000), "flags"),
                         (dict(pixel_per_world_unit=0.0), "pixel_per_world_unit"), (dict(pixel_per_world_unit=-3.0), "pixel_per_world_unit"),
                         (dict(pixel_per_world_unit=float("nan")), "pixel_per_world_unit"), (dict(pixel_per_world_unit=float("inf")), "pixel_per_world_unit"),
                         (dict(center=(float("nan"), 0.0)), "center"), (dict(center=(0.0, float("-inf"))), "center"),
                         (dict(radius=-0.001), "radius"), (dict(radius=float(np.nextafter(H, F(1)))), "radius"), (dict(radius=float("nan")), "radius"),
                         (dict(radius=float("inf")), "radius"),
                         (dict(min_pixel_radius=-0.5), "min_pixel_radius"), (dict(min_pixel_radius=4.001), "min_pixel_radius"),
                         (dict(min_pixel_radius=float("nan")), "min_pixel_radius"),
                         (dict(speed_scale=float("nan")), "speed_scale"), (dict(speed_scale=float("inf")), "speed_scale"),
                         (dict(width=1 << 14, height=1 << 14), "width"), (dict(width=1 << 28, height=1), "width"), (dict(width=0xFFFFFFFF, height=0xFFFFFFFF), "width")]:
            rc, msg = call(layer, **kw)
            assert rc == E and word in msg and msg.startswith(fn + ":"), (kw, rc, msg)
        assert call(layer, radius=hh)[0] == OK and call(layer, min_pixel_radius=4.0)[0] == OK and call(layer, speed_scale=-1.0)[0] == OK
        assert call(layer, width=0, height=5)[0] == OK and call(layer, width=7, height=0)[0] == OK  # a successful no-op
        assert call(layer, width=0, height=5, radius=-1.0)[0] == E
    # the messages of a view error are sphx_render's own
    plain = y.SphxContext()
    v = y.render_fit(32, 16)
    v.radius = -1.0
    o = _lib.SphxRenderOut(rgba=buf[2].ctypes.data)
    assert plain.L.sphx_render(plain.h, C.byref(v), 0, C.byref(o)) == E
    assert plain.L.sphx_last_error(plain.h).decode().split(": ", 1)[1] == call(False, radius=-1.0)[1].split(": ", 1)[1]
    plain.close()
    # inside an open multi step
    timer = y.TimeManager()
    vmax = m.step_begin(y.duration_as_secs_f32(timer.simulation_step_ns()))
    assert "sphx_multi_step_begin" in refused(NR, m.render, width=32, height=16)
    assert "sphx_multi_step_begin" in refused(NR, m.render_layer, width=32, height=16)
    m.step_finish(y.duration_as_secs_f32(timer.update_simulation_step(F(0.01), vmax)))
    assert m.render(width=32, height=16).shape == (16, 32, 4)
    # the tile call: flags, outputs
    tc = m.tile_context(1)
    v = y.render_fit(32, 16)
    lay = _lib.SphxRenderLayer(buf[0].ctypes.data, buf[1].ctypes.data, buf[2].ctypes.data)
    assert L.sphx_tile_render_layer(tc.h, C.byref(v), 2, C.byref(lay)) == E and "flags" in L.sphx_last_error(tc.h).decode()
    assert L.sphx_tile_render_layer(tc.h, C.byref(v), 0, C.byref(_lib.SphxRenderLayer())) == E and "no output" in L.sphx_last_error(tc.h).decode()
    assert L.sphx_tile_render_layer(tc.h, None, 0, C.byref(lay)) == E and L.sphx_tile_render_layer(tc.h, C.byref(v), 0, None) == E
    assert L.sphx_tile_render_layer(tc.h, C.byref(v), 0, C.byref(lay)) == OK
    # the Python wrappers
    with pytest.raises(TypeError):
        m.render(widht=3)
    with pytest.raises(ValueError):
        m.render(rgba=False)
    assert m.render(width=0, height=4, pixel_per_world_unit=10.0).shape == (4, 0, 4)
    m.close()


def test_solver_object_reaches_the_tiled_picture():
    w = y.FluidParticleWorld()
    w.reset_fluid(1.0)
    s = y.DFSPHMultiSolver(w, [0, 0])
    t = y.TimeManager()
    assert "sphx_multi_upload" in refused(_lib.ERR_NOT_READY, s.render, width=32, height=16)  # (the solver uploads with its first step)
    s.simulation_steps(w, t, 3, sync_world=True)
    view = rr.fit(160, 120, radius=0.015)
    img, own = s.render(owner=True, **view.fields())
    lay = s.render_layer(**view.fields())
    assert np.array_equal(lay["rgba"], img) and np.array_equal(lay["owner"], own)
    fl = own < BND
    assert fl.any() and set(np.unique(own[fl]).tolist()) <= set(range(N))
    s.close()


# ---- 7. one process per tile -----------------------------------------------------------------------------------------------------------------------
def test_rank_mode_layers_merge_to_the_in_process_picture(tmp_path):
    """Two processes over gloo: each rank draws its own layer without talking to the other; the parent merges them with
    yasph2d_amd.render_merge and gets the picture of the in-process 2-strip run of the same steps (tiling-invariant mode).
    sphx_multi_render in rank mode is refused and names the two calls to use instead."""
    steps = 12
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1", "--master-port", "29549",
           os.path.join(HERE, "render_multi_rank_worker.py"), str(tmp_path), str(steps)]
    p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    r = [np.load(tmp_path / f"rank{k}.npz") for k in range(2)]
    for k in range(2):
        assert int(r[k]["render_code"]) == _lib.ERR_INVALID_ARGUMENT
        msg = str(r[k]["render_msg"])
        assert "rank mode" in msg and "sphx_multi_render_layer" in msg and "sphx_render_merge" in msg, msg
    layers = [dict(key=r[k]["key"], owner=r[k]["owner"], rgba=r[k]["rgba"]) for k in range(2)]
    # each rank's layer shows the particles that rank owns, and only those
    for k in range(2):
        fl = layers[k]["owner"] < BND
        assert fl.any() and set(np.unique(layers[k]["owner"][fl]).tolist()) <= set(r[k]["ids"].tolist())
    merged = y.render_merge(layers)
    m = make_multi(2, invariant=True, strips=(0, quantile_cuts(cell_coord(POS, 0), 2)))  # (the worker's cut)
    timer = y.TimeManager()
    m.steps(timer, steps)
    assert timer.simulation_step_ns() == int(r[0]["dt_ns"])
    view = rr.fit(320, 240, radius=0.015)
    want = m.render_layer(**view.fields())
    assert same(merged, want)
    assert same(y.render_merge(layers[::-1]), want)  # (between the tiles of one run the order of the fold does not matter)
    img, own = m.render(owner=True, **view.fields())
    assert np.array_equal(merged["rgba"], img) and np.array_equal(merged["owner"], own)
    multi, not_lowest, not_highest = rm.seam_counts(layers)
    print("two ranks: %d pixels covered by both, winner not rank 0 at %d, not rank 1 at %d" % (multi, not_lowest, not_highest))
    assert multi >= 100 and not_lowest >= 20 and not_highest >= 20
    m.close()
