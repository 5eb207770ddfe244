"""Queries, contours, tracking, edits and the whole tiled service layer away from the reference app's constants: the sets `fine`
(h = 0.01, grid_min (-3, -7.5), oblique gravity), `tiny` (h = 0.0025000002) and `odd` (h = 0.18033393, fl(h fl(1/h)) != 1, grid_min
-500) of tests/constants_scenes.py, and `wide` (9 particles per cell) for the single-context queries.

These are the services where the constants enter a second time, on the host: the routing of points and appended records to the tile
that owns the cell, the lattice and pixel windows of a tile, the Morton key of the composite rule, the radius <= h refusal.  At h = 0.02
and grid_min -100 a host copy with 1 / h for cell_inv, a fused o + i * d, a default grid_min or a literal radius agrees with the device;
here it hands a point to two tiles or to none.

Per set one single context and one 2 x 2 MultiSolver (one device, halo 8, a re-partition every 4 steps), both in tiling-invariant mode at
fixed (2, 2) iterations, run the tiled scene (6000 particles drifting across the cuts) for 10 steps; all read-only services are asked on
these shared states, every mutating test makes its own copies.  Each answer is compared with the existing numpy reference given the
set's constants, and — tiled — with the single context's answer, byte for byte.  The inputs are those of tests/constants_services.py;
tests/test_constants_services_host.py proves without a GPU that they exercise what they claim, and the cheap conditions are repeated
here on the device's own state."""
import numpy as np
import pytest

import constants_scenes as cs
import constants_services as sv
import contour_reference as cr
import edit_reference as er
import multi_edit_reference as xref
import query_multi_reference as qm
import query_reference as qr
import render_reference as rr
import sample_reference as sr
import stats_reference as stref
import yasph2d_amd as y
from util import assert_bits_equal, assert_same_neighbors, step_pair
from yasph2d_amd import _lib
from yasph2d_amd.multi import MultiSolver

pytestmark = pytest.mark.gpu

F = np.float32
FIXED = (2, 2)
EXTRA_STEPS = 4
bits = qm.bits


def refused(code, fn, *args, **kw):
    with pytest.raises(y.SphxError) as e:
        fn(*args, **kw)
    assert e.value.code == code, str(e.value)
    return str(e.value)


def by_id(d, keys=("ids", "pos", "vel")):
    o = np.argsort(d["ids"], kind="stable")
    return {k: d[k][o] for k in keys}


def device_steps(ctx, timer, k, diam):
    for _ in range(k):
        vmax = ctx.step_begin(timer.simulation_step(), timer.law(diam))
        ctx.step_finish(y.duration_as_secs_f32(timer.update_simulation_step(diam, vmax)))


def new_context(name, scene):
    pos, vel, boundary = scene
    ctx = y.SphxContext(cs.params(name, fixed_iterations=FIXED))
    ctx.set_tiling_invariant(True)
    ctx.set_boundary(boundary)
    ctx.upload(pos, vel)
    return ctx


def new_multi(name, world=4, layout=_lib.LAYOUT_AUTO, params=None):
    m = MultiSolver(params if params is not None else cs.params(name, fixed_iterations=FIXED), devices=[0] * world, halo=cs.TILED_HALO, rebalance_every=4,
                    layout=layout)
    m.set_tiling_invariant(True)
    return m


def tiled_multi(name, scene, world=4):
    """the 2 x 2 run (or one tile) of the tiled scene, uploaded"""
    pos, vel, boundary = scene
    m = new_multi(name, world)
    if world == 4:
        xcuts, ycuts = cs.tile_cuts(name, pos)
        m.set_grid(xcuts, np.array(ycuts, np.uint32))
    m.set_boundary(boundary)
    m.upload(pos, vel)
    return m


def tile_states(m):
    """[(download, boundary)] of every tile, and query_multi_reference's form of the same"""
    states = qm.tile_states(m)
    tiles = []
    for k in range(len(states)):
        t = m.tile_context(k)
        tiles.append((t.download(), states[k]["boundary"]))
    return states, tiles


class Run:
    """One set's shared states: the single context and the 2 x 2 run after 10 steps, and what the references need of them."""

    def __init__(self, name, tiled=True):
        self.name, self.diam = name, cs.diameter(name)
        self.scene = cs.tiled_scene(name)
        self.n = len(self.scene[0])
        self.ctx = new_context(name, self.scene)
        self.timer = y.TimeManager()
        device_steps(self.ctx, self.timer, cs.TILED_STEPS, self.diam)
        self.K = sr.Constants(self.ctx.params, self.ctx.constants())
        d = self.ctx.download()
        assert not self.ctx.last_flags() & y.FLAG_STRAY_PARTICLES
        bxy, bid = self.ctx.download_boundary()
        self.st = dict(pos=d["pos"], vel=d["vel"], density=d["density"], ids=d["ids"], boundary=bxy, boundary_ids=bid)
        assert self.K.h == sv.h_of(name) and tuple(self.K.gmin) == tuple(sv.gmin_of(name)) and F(self.ctx.params.particle_radius) == sv.radius_of(name)
        self.m = None
        if tiled:
            self.m = tiled_multi(name, self.scene)
            self.rects0 = self.m.tile_rects()
            self.mtimer = y.TimeManager()
            for _ in range(cs.TILED_STEPS):
                self.m.step(self.mtimer, self.diam)
            self.rects = self.m.tile_rects()
            self.states, self.tiles = tile_states(self.m)
            self.maps = qm.boundary_maps(self.states, self.scene[2])
            self.whole = self.m.download()
        self.pts = sv.point_set(name, self.st["pos"], self.st["boundary"], self.rects if tiled else None)
        self._ref = {}

    def ref(self, radius, boundary):
        key = (float(radius), boundary)
        if key not in self._ref:
            self._ref[key] = qr.query32(self.K, self.st, self.pts, radius, boundary)
        return self._ref[key]

    def close(self):
        self.ctx.close()
        if self.m is not None:
            self.m.close()


@pytest.fixture(scope="module")
def _runs():
    made = {}

    def get(name):
        if name not in made:
            made[name] = Run(name, tiled=name in sv.TILED_SETS)
        return made[name]

    yield get
    for r in made.values():
        r.close()


@pytest.fixture(scope="module", params=sv.QUERY_SETS)
def single(request, _runs):
    """every set's single context (at `wide` there is no tiled run)"""
    return _runs(request.param)


@pytest.fixture(scope="module", params=sv.TILED_SETS)
def run(request, _runs):
    return _runs(request.param)


# ================================================================================================================ the two runs agree
def test_tiled_run_equals_the_single_context_and_particles_migrate(run):
    """test_tiles_at_fine's assertion at every set: ids, positions, velocities and the timer agree bit for bit by id.  Then the
    conditions of the CPU module on the device's own state: at least 1 % of the particles are owned by another tile than at upload,
    every tile owns at least 10 %, and every tile owns a particle further than the halo from every cut."""
    name, n = run.name, run.n
    a, ref = by_id(run.whole), by_id(run.st)
    np.testing.assert_array_equal(a["ids"], np.arange(n, dtype=np.uint32))
    assert_bits_equal(a["pos"], ref["pos"], "positions, 2 x 2 tiles at " + name)
    assert_bits_equal(a["vel"], ref["vel"], "velocities, 2 x 2 tiles at " + name)
    assert run.mtimer.simulation_step_ns() == run.timer.simulation_step_ns()
    info = run.m.info()
    assert info["owned_local"] == n and info["build_particles"] > n and info["rebalances"] >= 1, info
    before, after = sv.owned_tile(name, run.rects0, run.scene[0]), sv.owned_tile(name, run.rects, a["pos"])
    moved, sizes = int((before != after).sum()), np.bincount(after, minlength=4)
    # the tiles agree with the cell rule about who owns what
    for k, st in enumerate(run.states):
        mine = (st["ids"] >> 31) == 1
        assert np.array_equal(np.sort(st["ids"][mine] & np.uint32(0x7FFFFFFF)), np.nonzero(after == k)[0]), (name, k)
        cells = cs.cells(name, st["pos"][mine])
        x0, x1, y0, y1 = run.rects[k].tolist()
        far = np.ones(len(cells), bool)
        for axis, (lo, hi) in enumerate(((x0, x1), (y0, y1))):
            if lo > 0:
                far &= cells[:, axis] - lo >= cs.TILED_HALO
            if hi < 65536:
                far &= hi - 1 - cells[:, axis] >= cs.TILED_HALO
        assert far.any(), (name, k)
        assert (~mine).any(), (name, k)  # ghosts exist
    print("%s: %d of %d particles change tile, tiles own %s, rectangles %s -> %s" % (name, moved, n, sizes.tolist(), run.rects0.tolist(), run.rects.tolist()))
    assert moved >= 0.01 * n and sizes.min() >= 0.10 * n, (name, moved, sizes)


# ==================================================================================================================== single context
def test_query_against_the_reference(single):
    """ctx.query at h (the set's fp32 value), 0.9 h and 0.5 h, fluid and boundary, against query32 bit for bit; at 0.9 h and 0.5 h also
    against the search over all particles; nextafter(h, +inf) is refused."""
    import test_gpu_query as tq

    S, name = single, single.name
    answers = {}
    for boundary in (False, True):
        for r in sv.radii(name):
            got = S.ctx.query(S.pts, r, boundary=boundary)
            tq.assert_same(got, S.ref(r, boundary), "%s radius %g boundary %d" % (name, r, boundary))
            answers[(boundary, float(r))] = got
        for r in sv.radii(name)[1:]:
            brute = qr.brute32(S.st, S.pts, r, boundary=boundary)
            assert np.array_equal(np.sort(qr.pairs(answers[(boundary, float(r))])), np.sort(qr.pairs(brute))), (name, r, boundary)
    owner = qm.owner_of(S.K, S.rects, S.pts) if S.m is not None else None
    sv.point_conditions(name, S.pts, owner, answers)
    h = sv.h_of(name)
    assert "radius" in refused(_lib.ERR_INVALID_ARGUMENT, S.ctx.query, S.pts[:8], np.nextafter(h, F(np.inf)))
    assert S.ctx.query(S.pts, None)["count"] == answers[(False, float(h))]["count"]  # (radius None: the set's h)
    longest = int(np.diff(answers[(False, float(h))]["offsets"].astype(np.int64)).max())
    assert longest >= (28 if name == "wide" else 12), (name, longest)  # wide: the dense-cell lists


def test_select_against_the_reference(run):
    name = run.name
    R = sv.rectangles(name, run.st["pos"], run.rects)
    counts = sv.rectangle_conditions(name, run.st["pos"], run.rects, R)
    cases = [([R["cross"]], False), ([R["below"]], False), ([R["half"]], False), ([R["cross"], R["half"]], True), (list(R.values()), False)]
    for rects, outside in cases:
        ref = qr.select32(run.st["pos"], run.st["ids"], rects, outside)
        got = run.ctx.select(rects, outside)
        assert got["count"] == ref["count"] and np.array_equal(got["index"], ref["index"]) and np.array_equal(got["id"], ref["id"]), (name, rects, outside)
        tiled = run.m.select(rects, outside, by_id=True)
        assert tiled["count"] == ref["count"] and np.array_equal(tiled["id"], np.sort(ref["id"])), (name, rects, outside)
        ref_m = qr.select32(run.whole["pos"], run.whole["ids"], rects, outside)
        got_m = run.m.select(rects, outside)
        assert np.array_equal(got_m["id"], ref_m["id"]) and len(np.unique(got_m["id"])) == len(got_m["id"]), (name, rects, outside)
        for t, st in enumerate(run.states):
            e = got_m["tile"] == t
            word = st["ids"][got_m["slot"][e]]
            assert (word >> 31).all() and np.array_equal(word & np.uint32(0x7FFFFFFF), got_m["id"][e]), (name, t)
    assert len(np.unique(run.m.select([R["cross"]])["tile"])) == 4 and counts["below"] == 0


def test_contour_against_the_reference(run):
    """ctx.contour and m.contour on the lattice of spacing 0.6 h: contour32 over sample_grid's values (themselves sample32's), the
    polylines against contour_reference.chain, the tiled answers the single context's bytes, the owner of every node the cell rule's."""
    import test_gpu_contour as tc

    name = run.name
    lat = sv.lattice(name, run.st["pos"])
    x0, y0, dx, dy, nx, ny = lat
    owner = sv.node_owner(name, lat, run.rects)
    for field, iso in (("fraction", 0.5), ("density", 0.5 * float(cs.properties(name)["fluid_density"]))):
        what = "%s %s iso %g" % (name, field, iso)
        values, ref, dev = tc.check(run.ctx, run.st, lat, iso, y.KERNEL_WENDLAND_C2, field, what)
        grid = run.ctx.sample_grid((x0, y0), (dx, dy), (ny, nx), fields=(field,))
        assert np.array_equal(bits(grid[field]).ravel(), bits(values).ravel()), what
        sv.contour_conditions(name, lat, run.rects, ref)
        lines, closed = cr.lines_of(ref["segments"])
        dl, dc = y.contour_lines(dev["segments"])
        assert dc == [bool(c) for c in closed] and len(dl) == len(lines) and all(np.array_equal(bits(a), bits(b)) for a, b in zip(dl, lines)), what
        # the tiled run: the same lattice values, the same segments, every node answered by the tile of its cell
        g = run.m.sample_grid((x0, y0), (dx, dy), (ny, nx), fields=(field,), tiles=True)
        assert np.array_equal(bits(g[field]).ravel(), bits(values).ravel()), what + ": tiled lattice values"
        assert np.array_equal(g["tile"].reshape(ny, nx), owner), what + ": node owners"
        tiled = run.m.contour((x0, y0), (dx, dy), (ny, nx), iso=iso, field=field, tiles=True)
        assert tiled["count"] == ref["count"] and np.array_equal(tiled["cell"], ref["cell"]) and np.array_equal(bits(tiled["segments"]), bits(ref["segments"])), what
        cell = ref["cell"].astype(np.int64)
        assert np.array_equal(tiled["tile"], owner[cell // (nx - 1), cell % (nx - 1)].astype(np.int32)), what + ": tile of node 0"
    # the points of the queries through the samplers, tiled against single against sample32
    import test_gpu_sample as ts

    st = {k: run.st[k] for k in ("pos", "vel", "density", "boundary")}
    want = sr.sample32(run.K, st, run.pts, y.KERNEL_WENDLAND_C2)
    ts.assert_bits(run.ctx.sample(run.pts), want, name + ": sample")
    got = run.m.sample(run.pts, tiles=True)
    assert np.array_equal(got.pop("tile"), qm.owner_of(run.K, run.rects, run.pts)), name
    ts.assert_bits(got, want, name + ": tiled sample")


def test_track_and_download_by_id(run):
    name, n = run.name, run.n
    rng = np.random.default_rng(5)
    ids = np.concatenate([rng.choice(n, 300, replace=False), [0, n - 1, n, 2 * n + 7]]).astype(np.uint32)  # (the last two exist nowhere)
    order = np.argsort(run.st["ids"])
    for who in (run.ctx, run.m):
        who.track(ids)
        got = who.track_fetch()
        assert (got["slot"][-2:] == _lib.TRACK_ABSENT).all() and (bits(got["pos"][-2:]) == 0x7FC00000).all(), name
        for f in ("pos", "vel", "density"):
            assert np.array_equal(bits(got[f][:-2]), bits(run.st[f][order][ids[:-2]])), (name, f)
        all_ = who.download_by_id(0, n)
        assert all_["present"] == n
        for f in ("pos", "vel", "density"):
            assert np.array_equal(bits(all_[f]), bits(run.st[f][order])), (name, f)
        who.track([])
    run.ctx.track(ids)
    assert np.array_equal(run.st["ids"][run.ctx.track_fetch()["slot"][:-2]], ids[:-2])
    run.ctx.track([])
    run.m.track(ids)
    got = run.m.track_fetch()
    for t, st in enumerate(run.states):
        e = np.nonzero(got["tile"][:-2] == t)[0]
        assert np.array_equal(st["ids"][got["slot"][e]], ids[e] | np.uint32(0x80000000)), (name, t)
    assert np.array_equal(got["tile"][:-2], sv.owned_tile(name, run.rects, run.st["pos"][order][ids[:-2]]).astype(np.uint32))
    run.m.track([])


def test_recorders_agree(run):
    """a recorder over the 10 steps on a separately stepped pair (track_record before stepping): the tiled frames are the single
    context's, and the tile of every frame is the cell rule's at that frame"""
    name, n = run.name, run.n
    ids = np.arange(0, n, 17, dtype=np.uint32)
    ctx, m = new_context(name, run.scene), tiled_multi(name, run.scene)
    for who in (ctx, m):
        who.track(ids)
        who.track_record(cs.TILED_STEPS + 2)
    t1, t2 = y.TimeManager(), y.TimeManager()
    device_steps(ctx, t1, cs.TILED_STEPS, run.diam)
    rects = []
    for _ in range(cs.TILED_STEPS):
        m.step(t2, run.diam)
        rects.append(m.tile_rects())
    a, (b, tile) = ctx.track_frames(), m.track_frames(tiles=True)
    assert a.shape == (cs.TILED_STEPS, len(ids), 4) and np.array_equal(bits(a), bits(b)), name
    assert np.array_equal(bits(a[-1][:, :2]), bits(run.st["pos"][np.argsort(run.st["ids"])][ids])), name  # (the shared run's last frame)
    changed = 0
    for k in range(cs.TILED_STEPS):
        assert np.array_equal(tile[k], sv.owned_tile(name, rects[k], a[k][:, :2]).astype(np.uint32)), (name, k)
        changed += int((tile[k] != tile[0]).sum())
    assert changed > 0, name
    assert m.state_digest() == run.m.state_digest()  # recording leaves no trace in the run
    ctx.close()
    m.close()


def test_remove_and_append_equal_the_round_trip_and_the_oracle(run):
    """tests/test_gpu_edit.py's trio at the set: X edits on the device, Y makes the round trip through the host (edit_reference), the
    oracle of the set is edited with set_particles; 10 steps before and 4 lock-step steps after (util.step_pair, the set's diameter)."""
    name = run.name
    pos, vel, boundary = run.scene
    X, Y, O = y.SphxContext(cs.params(name)), y.SphxContext(cs.params(name)), cs.oracle(name)
    for c in (X, Y):
        c.set_boundary(boundary)
        c.upload(pos, vel)
    O.set_boundary(boundary)
    O.set_particles(pos, vel)
    tx, ty = y.TimeManager(), y.TimeManager()
    for s in range(cs.TILED_STEPS):
        step_pair(X, O, tx, run.diam, "%s step %d" % (name, s))
    device_steps(Y, ty, cs.TILED_STEPS, run.diam)
    assert tx.simulation_step_ns() == ty.simulation_step_ns()
    d = Y.download()
    R = sv.rectangles(name, d["pos"], run.rects)
    new, new_vel = (a[:81] for a in sv.appended_block(name, d["pos"], run.rects))  # (the block alone: nothing off the grid here)
    removed = X.remove([R["cross"]])
    first = X.append(new, new_vel)
    assert first == run.n
    p, v, ids, r = er.remove(d["pos"], d["vel"], d["ids"], [R["cross"]])
    assert r == removed and 0 < removed < run.n
    p, v, ids = er.append(p, v, ids, new, new_vel, first)
    Y.upload(p, v)
    po, vo = O.positions(), O.velocities()
    gone = er.removed_mask(po, [R["cross"]])
    O.set_particles(np.concatenate([po[~gone], new]), np.concatenate([vo[~gone], new_vel]))
    for s in range(EXTRA_STEPS):
        step_pair(X, O, tx, run.diam, "%s step %d after the edit" % (name, s))
    device_steps(Y, ty, EXTRA_STEPS, run.diam)
    dx, dy = X.download(), Y.download()
    for f, ref in (("pos", O.positions()), ("vel", O.velocities()), ("density", O.densities())):
        assert_bits_equal(dx[f], dy[f], "%s: %s, device edit against round trip" % (name, f))
        assert_bits_equal(dx[f], ref, "%s: %s against the oracle" % (name, f))
    assert_same_neighbors(X.download_neighbors(), O.neighbors())
    np.testing.assert_array_equal(dx["ids"], ids[dy["ids"]])
    assert not (O.neighbor_flags() & 2)
    X.close()
    Y.close()


# ========================================================================================================================= tiled run
def test_tiled_query_against_the_single_context_and_the_reference(run):
    name = run.name
    owner = qm.owner_of(run.K, run.rects, run.pts)
    assert np.bincount(owner, minlength=4).min() >= 32
    d, bid = run.st, run.st["boundary_ids"]
    for boundary in (False, True):
        ids = bid if boundary else d["ids"]
        for r in sv.radii(name):
            what = "%s radius %g boundary %d" % (name, r, boundary)
            got = run.m.query(run.pts, r, boundary=boundary, tiles=True)
            qm.assert_same(got, qm.reference(run.K, run.states, run.maps, owner, run.pts, r, boundary), what)
            one = run.ctx.query(run.pts, r, boundary=boundary)
            assert got["count"] == one["count"] and np.array_equal(got["offsets"], one["offsets"]), what
            assert np.array_equal(got["id"], one["id"]) and np.array_equal(bits(got["dist_sq"]), bits(one["dist_sq"])), what
            near = np.where(one["nearest"] != qm.NONE, ids[np.minimum(one["nearest"], len(ids) - 1)], qm.NONE)
            assert np.array_equal(got["nearest_id"], near) and np.array_equal(bits(got["nearest_dist_sq"]), bits(one["nearest_dist_sq"])), what
    assert "radius" in refused(_lib.ERR_INVALID_ARGUMENT, run.m.query, run.pts[:8], np.nextafter(sv.h_of(name), F(np.inf)))


def test_tiled_render_against_the_single_context_and_the_layers(run):
    name = run.name
    rect, views = sv.views(name, run.st["pos"], run.st["boundary"], run.rects)
    fitted = y.render_fit(160, 120, rect)
    assert (F(fitted.pixel_per_world_unit), tuple(F(c) for c in fitted.center)) == (views["fit"].pixel_per_world_unit, views["fit"].center)
    single = dict(pos=run.st["pos"], vel=run.st["vel"], boundary=run.st["boundary"])
    xy = np.concatenate([run.st["pos"], run.st["boundary"]])
    import render_multi_reference as rm

    for vname, view in views.items():
        what = "%s %s" % (name, vname)
        ref = rr.render32(single, view, sv.radius_of(name))
        img, own = run.ctx.render(**view.fields(), owner=True)
        assert np.array_equal(img, ref["rgba"]) and np.array_equal(own, ref["owner"]), what + ": single context"
        fluid = own < rr.BOUNDARY
        timg, town = run.m.render(owner=True, **view.fields())
        assert np.array_equal(timg, img), what + ": rgba"
        assert np.array_equal(town[fluid], run.st["ids"][own[fluid]]) and np.array_equal(town[~fluid], own[~fluid]), what + ": owners"
        layers = sv.tile_layers(name, run.tiles, view, [tuple(r) for r in run.rects.tolist()])  # (a tile draws the boundary of its cells)
        want = rm.merge(layers)
        got = run.m.render_layer(**view.fields())
        assert all(np.array_equal(got[k], want[k]) for k in ("key", "owner", "rgba")), what + ": layer"
        assert np.array_equal(want["rgba"], img), what
        for k in range(4):
            tl = run.m.tile_context(k).tile_render_layer(**view.fields())
            assert all(np.array_equal(tl[f], layers[k][f]) for f in ("key", "owner", "rgba")), "%s: tile %d" % (what, k)
        multi, not_lowest, not_highest = rm.seam_counts(layers)
        print("%s: %d pixels claimed by two tiles, winner not the lowest rank %d, not the highest %d" % (what, multi, not_lowest, not_highest))
        assert fluid.any() and sv.rect_margin_conditions(name, xy, view) > 0, what
        if vname == "fat":
            assert multi >= 20 and not_lowest >= 1 and not_highest >= 1, what
        if vname == "zoom":
            assert float(sv.radius_of(name)) * float(view.pixel_per_world_unit) >= 20.0
        if vname == "fit":  # another radius draws another picture: the set's radius is what the reference was given
            assert not np.array_equal(rr.render32(single, view, sv.APP_RADIUS)["owner"], ref["owner"])


def test_tiled_stats_against_the_single_context_and_the_reference(run):
    import test_gpu_stats_multi as tsm

    name, n = run.name, run.n
    R = sv.rectangles(name, run.st["pos"], run.rects)
    rects = [R["cross"], R["below"], R["half"], tsm.EVERYTHING]
    whole, tiles = run.m.stats(rects, per_tile=True)
    want = tsm.check_all(whole, run.whole, rects, name + ", tiled")
    single = run.ctx.stats(rects)
    tsm.check_all(single, run.st, rects, name + ", single")
    for r in range(len(rects) + 1):
        for k in stref.EXACT:
            assert stref.bits(single[r][k]) == stref.bits(whole[r][k]), (name, r, k)
        for k in stref.SUMS:  # two device sums of one exact value: each within the header's n 2^-52 sum |t|
            a, b, ab = np.atleast_1d(single[r][k]), np.atleast_1d(whole[r][k]), np.atleast_1d(want[r]["abs_" + k])
            for j in range(len(a)):
                assert abs(float(a[j]) - float(b[j])) <= 2.0 * want[r]["n_" + k] * stref.U * ab[j], (name, r, k, j)
    c = whole["count"].tolist()
    assert c[0] == n == c[4] and 0 < c[1] < n and c[2] == 0 and 0 < c[3] < n, (name, c)
    assert (tiles[:, 1]["count"] > 0).all() and int(tiles[:, 0]["count"].sum()) == n  # the rectangle over the crossing meets every tile
    own = sv.owned_tile(name, run.rects, run.whole["pos"])
    for k in range(4):
        tsm.check_all(tiles[k], tsm.subset(run.whole, own == k), rects, "%s, tile %d" % (name, k))
    assert tsm.fold(tiles).tobytes() == whole.tobytes()


def test_tiled_state_into_other_tilings(run):
    """m.save_state() of the 2 x 2 run loaded into 2 strips and into one tile of the same parameter block, 4 more steps: the
    uninterrupted 2 x 2 run by id, bit for bit, with equal digests; a multi made with default_params() refuses the parts."""
    import test_gpu_state as tstate

    name = run.name
    blob = run.m.save_state()
    digest = run.m.state_digest()
    ends = []
    for world, layout in ((2, _lib.LAYOUT_STRIPS), (1, _lib.LAYOUT_AUTO)):
        k = new_multi(name, world, layout)
        k.load_state(blob)
        assert k.state_digest() == digest, (name, world)
        t = tstate.timer_like(run.mtimer)
        for _ in range(EXTRA_STEPS):
            k.step(t, run.diam)
        ends.append((by_id(k.download()), k.state_digest(), t.simulation_step_ns()))
        k.close()
    m = tiled_multi(name, run.scene)  # the uninterrupted run
    t = y.TimeManager()
    for _ in range(cs.TILED_STEPS):
        m.step(t, run.diam)
    assert m.state_digest() == digest and t.simulation_step_ns() == run.mtimer.simulation_step_ns()
    for _ in range(EXTRA_STEPS):
        m.step(t, run.diam)
    want, wd = by_id(m.download()), m.state_digest()
    assert wd != digest
    for (got, gd, ns), world in zip(ends, (2, 1)):
        assert np.array_equal(got["ids"], want["ids"]), (name, world)
        assert_bits_equal(got["pos"], want["pos"], "%s: positions, %d tiles after the load" % (name, world))
        assert_bits_equal(got["vel"], want["vel"], "%s: velocities, %d tiles after the load" % (name, world))
        assert gd == wd and ns == t.simulation_step_ns(), (name, world)
    m.close()
    app = MultiSolver(y.default_params(fixed_iterations=FIXED), devices=[0, 0], halo=cs.TILED_HALO, rebalance_every=4)
    app.set_tiling_invariant(True)
    from util import lattice_scene

    pos, boundary = lattice_scene(257, 37)
    app.set_boundary(boundary)
    app.upload(pos)
    before = app.state_digest()
    refused(_lib.ERR_INVALID_ARGUMENT, app.load_state, blob)
    assert app.state_digest() == before
    app.close()


def test_tiled_remove_and_append(run):
    """m.remove (the rectangle over the crossing of the cuts) then m.append (a block that straddles the x cut, three particles off the
    grid): the removed and the new ids against edit_reference and multi_edit_reference.route; 4 steps later the run equals a one-tile
    multi given the same edits, by id, bit for bit."""
    name, n = run.name, run.n
    ends = []
    for world in (4, 1):
        m = tiled_multi(name, run.scene, world)
        t = y.TimeManager()
        for _ in range(cs.TILED_STEPS):
            m.step(t, run.diam)
        d = by_id(m.download())
        R = sv.rectangles(name, run.st["pos"], run.rects)
        new, new_vel = sv.appended_block(name, run.st["pos"], run.rects)
        gone = er.removed_mask(d["pos"], [R["cross"]])
        want_removed = m.select([R["cross"]], by_id=True)["id"]
        assert np.array_equal(want_removed, d["ids"][gone])
        removed = m.remove([R["cross"]])
        assert removed == int(gone.sum()) and 0 < removed < n
        first = m.append(new, new_vel)
        assert first == n
        p, v, ids = er.append(d["pos"][~gone], d["vel"][~gone], d["ids"][~gone], new, new_vel, first)
        after = by_id(m.download())
        assert np.array_equal(after["ids"], ids) and np.array_equal(bits(after["pos"]), bits(p)) and np.array_equal(bits(after["vel"]), bits(v)), (name, world)
        if world == 4:  # every new record lives in the tile the routing rule names
            rects = m.tile_rects()
            route = xref.route(new, [tuple(r) for r in rects.tolist()], sv.gmin_of(name), sv.h_of(name))
            assert len(np.unique(route[:-3])) >= 2 and (route >= 0).all(), (name, route)
            m.track(np.arange(first, first + len(new), dtype=np.uint32))
            assert np.array_equal(m.track_fetch()["tile"], route.astype(np.uint32)), name
            m.track([])
        for _ in range(EXTRA_STEPS):
            m.step(t, run.diam)
        ends.append((by_id(m.download()), t.simulation_step_ns()))
        m.close()
    (a, ta), (b, tb) = ends
    assert ta == tb and np.array_equal(a["ids"], b["ids"]) and len(a["ids"]) == n - removed + len(new)
    assert_bits_equal(a["pos"], b["pos"], name + ": positions, 2 x 2 against one tile after the edits")
    assert_bits_equal(a["vel"], b["vel"], name + ": velocities, 2 x 2 against one tile after the edits")
