"""The services away from the reference app's constants, the part that needs no GPU.  tests/test_gpu_constants_services.py asks the
device for neighbour queries, selections, contours, pictures, statistics, edits and the tiled services at the parameter sets `fine`,
`tiny`, `odd` (and `wide`) of tests/constants_scenes.py; this module proves with the oracle and the numpy references alone that the
inputs it uses (tests/constants_services.py) exercise what they claim, so that the GPU module cannot pass on an empty case:

(1) conditions — particles change tile within the run, every tile is populated and owns particles no other tile holds as ghosts, the
    points reach every tile, the clamped cells and both empty and non-empty lists, the contour crosses both cut directions, two tiles
    claim common pixels with fluid owners, the rectangles select some particles and not all;
(2) sensitivity — every host-side rule (the owner of a point, the route of an appended record, the Morton key, the layer, the split,
    the lattice window), evaluated with the app's constants (h = 0.02, grid_min (-100, -100), radius 0.005) on the same inputs, gives
    another answer: a hard-coded constant in the library would fail the GPU comparison, not pass it;
(3) the host drivers of the routing rule, the contour apron and the render window at the three sets' constants, passed as fp32 bit
    patterns.

Figures of the oracle's run (6000 particles, drift (1500, 900) spacings per second, 10 steps at fixed (2, 2), tiling-invariant order):
particles that change tile 384 / 381 / 381 (fine / tiny / odd); the smallest tile owns 972 / 884 / 980; the fewest particles further
than the halo from every cut 220 / 84 / 228."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import constants_scenes as cs
import constants_services as sv
import contour_reference as cr
import multi_edit_reference as xref
import query_multi_reference as qm
import query_reference as qr
import render_multi_reference as rm
import render_reference as rr
import sample_reference as sr

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "yasph2d_amd", "csrc")
_states = {}


def tiled_state(name):
    """The tiled scene in the oracle: tiling-invariant order, fixed (2, 2) iterations, the adaptive timer at the set's diameter, 10 steps.
    Arrays in the oracle's own order (what a download would give), plus the upload and the 2 x 2 rectangles cut from it."""
    if name not in _states:
        pos0, vel0, boundary = cs.tiled_scene(name)
        o = cs.oracle(name)
        o.set_tiling_invariant(True)
        o.set_fixed_iterations(2, 2)
        o.set_boundary(boundary)
        o.set_particles(pos0, vel0)
        for _ in range(cs.TILED_STEPS):
            o.dfsph_step()
        rects = cs.tile_rects(*cs.tile_cuts(name, pos0))
        _states[name] = dict(pos0=pos0, vel0=vel0, boundary=o.boundary(), boundary_ids=o.boundary_ids(), rects=rects, pos=o.positions(),
                             vel=o.velocities(), ids=o.ids(), density=o.densities())
    return _states[name]


def constants(name):
    return sr.Constants(cs.params(name))


# ------------------------------------------------------------------------------------------------------------------ 1. conditions
@pytest.mark.parametrize("name", sv.TILED_SETS)
def test_particles_migrate_and_every_tile_has_an_interior(name):
    s = tiled_state(name)
    n, rects = len(s["pos"]), s["rects"]
    assert np.isfinite(s["pos"]).all() and np.isfinite(s["vel"]).all()
    by_id = np.argsort(s["ids"])
    before, after = sv.owned_tile(name, rects, s["pos0"]), sv.owned_tile(name, rects, s["pos"][by_id])
    moved = int((before != after).sum())
    sizes = np.bincount(after, minlength=4)
    c = cs.cells(name, s["pos"][by_id])
    interior = []
    for t, (x0, x1, y0, y1) in enumerate(rects.tolist()):
        cc = c[after == t]
        far = np.ones(len(cc), bool)
        for axis, (a, b) in enumerate(((x0, x1), (y0, y1))):
            if a > 0:
                far &= cc[:, axis] - a >= cs.TILED_HALO
            if b < 65536:
                far &= b - 1 - cc[:, axis] >= cs.TILED_HALO
        interior.append(int(far.sum()))
    print("%s: %d of %d particles change tile, tiles own %s, further than the halo from every cut %s" % (name, moved, n, sizes.tolist(), interior))
    assert moved >= 0.01 * n, (name, moved)
    assert sizes.min() >= 0.10 * n, (name, sizes)
    assert min(interior) >= 1, (name, interior)
    # the block is 32 to 40 cells wide and lies away from the app's cells (around 5000)
    span = c.max(0) - c.min(0) + 1
    assert (span >= 25).all() and (span <= 48).all() and not ((c > 4900) & (c < 5100)).any(), (name, span)


@pytest.mark.parametrize("name", sv.QUERY_SETS)
def test_points_reach_every_tile_the_clamped_cells_and_both_kinds_of_list(name):
    s = tiled_state(name)
    K = constants(name)
    rects = s["rects"] if name in sv.TILED_SETS else None
    pts = sv.point_set(name, s["pos"], s["boundary"], rects)
    answers = {(b, float(r)): qr.query32(K, s, pts, r, boundary=b) for b in (False, True) for r in sv.radii(name)}
    owner = qm.owner_of(K, rects, pts) if rects is not None else None
    off_grid, figures = sv.point_conditions(name, pts, owner, answers)
    print("%s: %d points, %d off the grid, (non-empty, empty) per (boundary, radius): %s" % (name, len(pts), off_grid, figures))
    full = answers[(False, float(sv.radii(name)[0]))]
    longest = int(np.diff(full["offsets"].astype(np.int64)).max())
    assert (full["dist_sq"] == 0).sum() >= (160 if rects is not None else 0)  # the points that sit on particles
    # a disc of radius h holds pi (h / spacing)^2 particles of a lattice: 12.6 at smoothing factor 2, 28.3 at `wide` (9 per cell)
    assert longest >= (28 if name == "wide" else 12), (name, longest)
    # completeness below 0.9 h: the box rule is the search over all particles
    for r in sv.radii(name)[1:]:
        for b in (False, True):
            assert np.array_equal(np.sort(qr.pairs(answers[(b, float(r))])), np.sort(qr.pairs(qr.brute32(s, pts, r, boundary=b)))), (name, r, b)
    if rects is None:
        return
    # the owner is the cell rule of the set: restated independently (constants_scenes.cells), and another one at the app's constants
    assert np.array_equal(owner, sv.owned_tile(name, rects, pts))
    other = qm.owner_of(sv.app_constants(), rects, pts)
    assert (other != owner).sum() >= 100, name


@pytest.mark.parametrize("name", sv.TILED_SETS)
def test_rectangles_and_the_appended_block(name):
    s = tiled_state(name)
    rects = s["rects"]
    R = sv.rectangles(name, s["pos"], rects)
    counts = sv.rectangle_conditions(name, s["pos"], rects, R)
    print("%s: cross %d, below %d, half %d of %d" % (name, counts["cross"], counts["below"], counts["half"], len(s["pos"])))
    # the appended block straddles the x cut, and three particles go below grid_min: the route of the set, and the app's
    new, _ = sv.appended_block(name, s["pos"], rects)
    h, gm = sv.h_of(name), sv.gmin_of(name)
    route = xref.route(new, [tuple(r) for r in rects.tolist()], gm, h)
    assert np.array_equal(route, sv.owned_tile(name, rects, new))
    per = np.bincount(route[:-3], minlength=4)
    assert (per > 0).sum() >= 2 and per[:2].sum() > 0 and per[2:].sum() > 0, (name, per)     # both columns
    assert (new[-3:] < gm).any(1).all() and (cs.cells(name, new[-3:]) == 0).any(1).all()      # clamped to cell 0 on an axis
    assert qr.select32(new, np.arange(len(new)), [R["below"]])["count"] == 1                  # (one of the three lies in `below`)
    other = xref.route(new, [tuple(r) for r in rects.tolist()], sv.APP_GRID_MIN, sv.APP_H)
    assert (other != route).any(), name
    # free space: no fluid particle within 3 h of the block
    d = np.abs(new[:81, None, :].astype(np.float64) - s["pos"][None, :, :]).max(2).min()
    assert d > 3 * float(h), (name, d)


@pytest.mark.parametrize("name", sv.TILED_SETS)
def test_contour_lattice_crosses_both_cut_directions(name):
    s = tiled_state(name)
    K = constants(name)
    rects = s["rects"]
    lat = sv.lattice(name, s["pos"])
    assert 2000 <= lat[4] * lat[5] <= 8000, lat
    pts = sr.lattice_points(*lat)
    for field, iso in (("fraction", 0.5), ("density", 0.5 * float(cs.properties(name)["fluid_density"]))):
        values = sr.sample32(K, s, pts, sr.KERNEL_WENDLAND)[field]
        ref = cr.contour32(values, *lat, iso)
        figures = sv.contour_conditions(name, lat, rects, ref)
        print("%s %s iso %g: %d segments, %d cells across the x cut, %d across a y cut, longest chain %d" % ((name, field, iso) + figures))
    # the windows of the app's cell grid are others
    wins = sv.lattice_windows(lat, rects, sv.h_of(name), sv.gmin_of(name))
    assert wins != sv.lattice_windows(lat, rects, sv.APP_H, sv.APP_GRID_MIN), name


@pytest.mark.parametrize("name", sv.TILED_SETS)
def test_render_views_put_the_seams_under_load(name):
    s = tiled_state(name)
    rects = [tuple(r) for r in s["rects"].tolist()]
    h, gm, radius = sv.h_of(name), tuple(sv.gmin_of(name)), sv.radius_of(name)
    tiles = rm.split(s, rects, h, gm)
    assert sum(len(t["pos"]) for t, _ in tiles) == len(s["pos"]) and sum(len(b) for _, b in tiles) == len(s["boundary"])
    rect, views = sv.views(name, s["pos"], s["boundary"], rects)
    single = dict(pos=s["pos"], vel=s["vel"], boundary=s["boundary"])
    xy = np.concatenate([s["pos"], s["boundary"]])
    shared = 0
    for vname, view in views.items():
        layers = sv.tile_layers(name, tiles, view)
        multi, not_lowest, not_highest = rm.seam_counts(layers)
        want = rm.merge(layers)
        one = rr.render32(single, view, radius)
        fluid = one["owner"] < rr.BOUNDARY
        # the composite of the tiles' layers is the single picture (ids for indices)
        assert np.array_equal(want["rgba"], one["rgba"]) and np.array_equal(want["owner"][fluid], s["ids"][one["owner"][fluid]]), (name, vname)
        assert np.array_equal(want["owner"][~fluid], one["owner"][~fluid])
        discs = sv.rect_margin_conditions(name, xy, view)
        print("%s %s: %d pixels claimed by two tiles (winner not the lowest rank %d, not the highest %d), %d fluid pixels, %d discs on the image"
              % (name, vname, multi, not_lowest, not_highest, int(fluid.sum()), discs))
        assert fluid.any() and discs > 0, (name, vname)
        if vname == "fat":
            assert multi >= 20 and not_lowest >= 1 and not_highest >= 1, (name, multi, not_lowest, not_highest)
        if vname == "zoom":
            assert float(radius) * float(view.pixel_per_world_unit) >= 20.0
        shared += multi
        # the app's constants draw and key otherwise
        if vname == "fit":
            assert not np.array_equal(rr.render32(single, view, sv.APP_RADIUS)["owner"], one["owner"]), name
            app_layers = [rm.layer32(t, b, view, particle_radius=radius) for t, b in tiles]  # (h and grid_min of the app)
            assert any(not np.array_equal(a["key"], l["key"]) for a, l in zip(app_layers, layers)), name
    assert shared >= 1
    assert not np.array_equal(rm.cell_keys(s["pos"], h, gm), rm.cell_keys(s["pos"]))
    app_tiles = rm.split(s, rects)
    assert [len(t["pos"]) for t, _ in app_tiles] != [len(t["pos"]) for t, _ in tiles]


# ------------------------------------------------------------------------------------------- 3. the host drivers at the sets' constants
def bits(v):
    return "%08x" % int(np.array(v, F).view(np.uint32))


def grid_args(name):
    gm = sv.gmin_of(name)
    return [bits(gm[0]), bits(gm[1]), bits(sv.h_of(name))]


def build(tmp_path_factory, stem):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to compile the host drivers"
    exe = str(tmp_path_factory.mktemp(stem) / stem)
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(ROOT, "tests", stem + ".cpp"), "-o", exe])

    def run(*args):
        r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
        return r.returncode, r.stdout, r.stderr

    return run


@pytest.fixture(scope="module")
def edit_driver(tmp_path_factory):
    return build(tmp_path_factory, "multi_edit_driver")


@pytest.fixture(scope="module")
def contour_driver(tmp_path_factory):
    return build(tmp_path_factory, "contour_merge_driver")


@pytest.fixture(scope="module")
def render_driver(tmp_path_factory):
    return build(tmp_path_factory, "render_merge_driver")


@pytest.mark.parametrize("name", sv.TILED_SETS)
def test_routing_rule_at_the_sets_constants(edit_driver, name):
    """csrc/sphx_multi_edit.hpp: the hand cases of the routing section on the set's cell grid, then the scene's own records — the
    appended block, the points of the queries, the particles — routed by the header and by multi_edit_reference.route."""
    rc, out, err = edit_driver("routing", *grid_args(name))
    assert rc == 0 and out.startswith("ok ") and err == "", (out[-2000:], err[-2000:])
    s = tiled_state(name)
    rects = [tuple(r) for r in s["rects"].tolist()]
    new, _ = sv.appended_block(name, s["pos"], s["rects"])
    pts = sv.point_set(name, s["pos"], s["boundary"], s["rects"])
    rec = np.ascontiguousarray(np.concatenate([new, pts[(np.abs(pts) < 1e30).all(1)], s["pos"][::7]]), F)
    want = xref.route(rec, rects, sv.gmin_of(name), sv.h_of(name))
    args = grid_args(name) + [len(rects)] + [v for r in rects for v in r] + ["%08x" % w for w in rec.view(np.uint32).reshape(-1)]
    rc, out, err = edit_driver("routebits", *args)
    assert rc == 0 and err == "", err[-2000:]
    assert [int(v) for v in out.split()] == want.tolist()
    assert set(want.tolist()) == {0, 1, 2, 3}


@pytest.mark.parametrize("name", sv.TILED_SETS)
def test_contour_apron_at_the_sets_constants(contour_driver, name):
    rc, out, err = contour_driver("apron", *grid_args(name))
    assert rc == 0 and out.startswith("ok ") and err == "", (out[-2000:], err[-2000:])
    assert int(out.split()[1]) >= 32


@pytest.mark.parametrize("name", sv.TILED_SETS)
def test_render_window_at_the_sets_constants(render_driver, name):
    rc, out, err = render_driver("window", *grid_args(name))
    print(out)
    assert rc == 0 and "ok window" in out and "FAILED" not in out and err == "", out[-3000:] + err[-3000:]
