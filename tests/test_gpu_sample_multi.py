"""Sampling the fields of a tiled run on the device (include/sphx.h, "sampling the fields of a tiled run"): sphx_multi_sample_points,
sphx_multi_sample_grid and the fold of the ranks' parts.  The expected values never come from the calls under test: they are the
float32 restatement of the sampling contract (tests/sample_reference.py) over the answering tile's own downloads, or the single context
in tiling-invariant mode.  Everything is compared as bits.  All scenes are the dam break of tests/util.py at scale 1.0 (4 050
particles, every tile on device 0) with small halos and a re-partition every 4 steps, so that ghosts, migration and moving cuts really
happen.  The host side (lattice windows, the fold) is checked without a GPU in tests/test_sample_multi_host.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import multi_state_reference as mref
import sample_reference as sr
import yasph2d_amd as y
from util import dam_break
from yasph2d_amd import _lib
from yasph2d_amd.multi import MultiSolver

pytestmark = pytest.mark.gpu

F = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
POS, BOUNDARY = dam_break(1.0)
N = len(POS)
H = F(0.02)
DIAM = F(0.01)
KINDS = (y.KERNEL_WENDLAND_C2, y.KERNEL_POLY6, y.KERNEL_SPIKY)
STEP_FIELDS = tuple(k for k, _ in _lib.SphxStepStats._fields_)
# the fluid lies in the cell columns 5005 .. 5029 at t = 0: the last of these three strips (x >= 1.2, more than a halo away) holds the
# right-hand walls and no fluid, not even a ghost
THREE_STRIPS = (0, [0, 5017, 5060, 65536])
TILINGS = [(1, None), (2, None), (4, None), (3, THREE_STRIPS)]
TILING_IDS = ["one tile", "2 strips", "2x2", "3 strips, one without fluid"]
LATTICE = (F(-0.07), F(-0.09), F(0.0413), F(0.0391), 57, 71)  # x0, y0, dx, dy, nx, ny: over the scene rectangle, in and out of the fluid


def bits(a):
    a = np.ascontiguousarray(a)
    return a if a.dtype == np.uint32 else a.view(np.uint32)


def refused(code, fn, *args, **kw):
    with pytest.raises(y.SphxError) as e:
        fn(*args, **kw)
    assert e.value.code == code, str(e.value)
    return str(e.value)


def new_multi(world, strips=None, params=None, halo=10, rebalance_every=4, invariant=False, **kw):
    m = MultiSolver(params if params is not None else y.default_params(), devices=[0] * world, halo=halo, rebalance_every=rebalance_every, **kw)
    if invariant:
        m.set_tiling_invariant(True)
    if strips is not None:
        m.set_strips(*strips)
    m.set_boundary(BOUNDARY)
    return m


def tile_states(m):
    """every local tile's own arrays, ghosts included, and its clipped boundary: what the answering tile computes from"""
    out = []
    for k in range(m.info()["local_tiles"]):
        t = m.tile_context(k)
        d = t.download()
        out.append(dict(pos=d["pos"], vel=d["vel"], density=d["density"], boundary=t.download_boundary()[0], ids=d["ids"]))
    return out


def consts_of(m, params=None):
    return sr.Constants(params if params is not None else m.params, m.tile_context(0).constants())


def cell_centre(c):
    return (F(-100.0) + (F(c) + F(0.5)) * H).astype(F)


def point_set(rects, states, seed=7):
    """the lattice over the scene; points exactly on particles; the first and last owned cell column and row on both sides of every
    cut, also shifted by +-h; points beside the right wall; far-away, infinite and NaN points"""
    rng = np.random.default_rng(seed)
    pos = np.concatenate([s["pos"][(s["ids"] >> 31) == 1] for s in states])  # the owned particles of all tiles: the fluid
    pts = [sr.lattice_points(*LATTICE), pos[rng.choice(len(pos), 400, replace=False)]]
    ys = (F(0.55) + np.arange(64, dtype=F) * F(0.0193)).astype(F)  # through the fluid column and above it
    xs = (F(0.05) + np.arange(40, dtype=F) * F(0.0171)).astype(F)
    for x0, x1, y0, y1 in rects.tolist():
        for c in (x0, x1):
            if 0 < c < 65536:  # a vertical cut: the last column of the one side, the first of the other
                for col in (c - 1, c):
                    for shift in (F(0.0), H, -H):
                        pts.append(np.stack([np.full(len(ys), cell_centre(col) + shift, F), ys], -1))
        for c in (y0, y1):
            if 0 < c < 65536:
                for row in (c - 1, c):
                    for shift in (F(0.0), H, -H):
                        pts.append(np.stack([xs, np.full(len(xs), cell_centre(row) + shift, F)], -1))
    wall = BOUNDARY[BOUNDARY[:, 0] > F(1.3)]  # (beyond the last cut of THREE_STRIPS)
    pts.append((wall[rng.choice(len(wall), 200, replace=False)] + rng.normal(0, 0.007, (200, 2))).astype(F))
    pts.append(np.array([[1e6, 1e6], [-1e30, 0.5], [np.nan, 0.5], [0.5, np.nan], [np.inf, 0.5], [-np.inf, -np.inf], [-200.0, -200.0],
                         [3.4e38, -3.4e38]], F))
    return np.ascontiguousarray(np.concatenate(pts), F)


def owner_of(K, rects, pts):
    """the tile whose rectangle holds cells_of(q): exactly one per point"""
    c = sr.cells_of(K, pts)
    inside = np.stack([(c[:, 0] >= r[0]) & (c[:, 0] < r[1]) & (c[:, 1] >= r[2]) & (c[:, 1] < r[3]) for r in rects.tolist()], 0)
    assert (inside.sum(0) == 1).all(), "the rectangles do not partition the cell domain"
    return inside.argmax(0).astype(np.int32)


def reference(K, states, owner, pts, kind):
    """sample32 over the answering tile's own download and boundary, tile by tile"""
    ref = dict(density=np.zeros(len(pts), F), fraction=np.zeros(len(pts), F), velocity=np.zeros((len(pts), 2), F), count=np.zeros(len(pts), np.uint32))
    for t, st in enumerate(states):
        idx = np.nonzero(owner == t)[0]
        if len(idx):
            r = sr.sample32(K, st, pts[idx], kind)
            for f in ref:
                ref[f][idx] = r[f]
    return ref


def assert_bits(dev, ref, what):
    for f in dev:
        if f == "tile":
            continue
        a, b = bits(dev[f]), bits(ref[f])
        assert a.shape == b.shape and np.array_equal(a, b), "%s: %s differs at %d points" % (what, f, int((a != b).any(-1).sum() if a.ndim > 1 else (a != b).sum()))


def snapshot(m, what):
    """everything the device says about one state, taken while the multi is in it"""
    rects, states = m.tile_rects(), tile_states(m)
    pts = point_set(rects, states)
    s = dict(what=what, rects=rects, states=states, pts=pts, full={}, alone={}, pair={}, grid={})
    for kind in KINDS:
        s["full"][kind] = m.sample(pts, kind, tiles=True)
        s["alone"][kind] = {f: m.sample(pts, kind, fields=(f,)) for f in sr.FIELDS}
        s["pair"][kind] = m.sample(pts, kind, fields=("density", "velocity"))
        s["grid"][kind] = m.sample_grid(LATTICE[:2], LATTICE[2:4], (LATTICE[5], LATTICE[4]), kind, tiles=True)
    return s


@pytest.fixture(scope="module", params=TILINGS, ids=TILING_IDS)
def run40(request):
    """default mode, after the upload and after 40 adaptive steps with a re-partition every 4: (world, multi, constants, snapshots)"""
    world, strips = request.param
    m = new_multi(world, strips)
    m.upload(POS)
    snaps = [snapshot(m, "after the upload")]
    m.steps(y.TimeManager(), 40)
    snaps.append(snapshot(m, "after 40 steps"))
    if world > 1:
        assert m.info()["rebalances"] >= 1, m.info()
    yield world, m, consts_of(m), snaps
    m.close()


# ---- 1. against the answering tile -----------------------------------------------------------------------------------------------------------
def test_bit_identical_to_the_answering_tiles_own_arrays(run40):
    world, m, K, snaps = run40
    for s in snaps:
        what = "%d tiles, %s" % (world, s["what"])
        assert len(s["rects"]) == world and len(s["states"]) == world
        owner = owner_of(K, s["rects"], s["pts"])
        if world > 1:
            assert len(np.unique(owner)) == world, what + ": the point set does not reach every tile"
        for kind in KINDS:
            ref = reference(K, s["states"], owner, s["pts"], kind)
            full = s["full"][kind]
            assert full["tile"].dtype == np.int32 and np.array_equal(full["tile"], owner), what + ": tile is not the rectangle of cells_of(q)"
            assert_bits(full, ref, "%s kind %d" % (what, kind))
            for f in sr.FIELDS:
                assert_bits(s["alone"][kind][f], {f: ref[f]}, "%s kind %d %s alone" % (what, kind, f))
            assert_bits(s["pair"][kind], ref, "%s kind %d density + velocity" % (what, kind))
            # far and non-finite points: zeros, answered by the tile of their saturated cell
            tail = slice(len(s["pts"]) - 8, len(s["pts"]))
            assert not full["density"][tail].any() and not full["count"][tail].any() and not full["fraction"][tail].any()
        assert full["count"].max() >= 8 and (full["fraction"] > 0.9).any()  # (the points do meet the fluid: about ten particles within h)


def test_the_fluid_less_strip_answers_from_its_static_grid():
    """three strips whose last holds walls and no fluid, not even a ghost: that tile has no dynamic grid and answers from its walls"""
    m = new_multi(*TILINGS[3])
    m.upload(POS)
    states, rects = tile_states(m), m.tile_rects()
    assert len(states[2]["pos"]) == 0 and len(states[2]["boundary"]) > 0, "the last strip was meant to hold walls and no fluid"
    pts = point_set(rects, states)
    K = consts_of(m)
    owner = owner_of(K, rects, pts)
    there = owner == 2
    assert there.sum() >= 200
    for kind in KINDS:
        d = m.sample(pts, kind, tiles=True)
        assert np.array_equal(d["tile"], owner)
        assert (d["density"][there] > 0).sum() >= 100 and not d["count"][there].any() and not d["fraction"][there].any() and not d["velocity"][there].any()
        assert_bits({f: v[there] for f, v in d.items()}, sr.sample32(K, states[2], pts[there], kind), "the fluid-less strip, kind %d" % kind)
    m.close()


def test_a_fluid_less_tile_steps_with_fixed_iteration_counts():
    """The step of a tile without particles: with fixed 2 + 2 iterations both warm starts fire from the second step on.  The re-grid of
    such a tile launches a build over the slots an exchange could have filled and leaves that build's hand-off; its iteration used to
    return without taking it and the next warm start refused ("warm start after sphx_sub_regrid_div")."""
    m = new_multi(*TILINGS[3], params=y.default_params(fixed_iterations=(2, 2)), halo=16, invariant=True)
    m.upload(POS)
    assert m.tile_context(2).n == 0
    timer = y.TimeManager()
    stats = [m.step(timer) for _ in range(6)]
    assert all(st["density_iterations"] == 2 and st["divergence_iterations"] == 2 for st in stats)
    assert sum(st["warmstart_density"] + st["warmstart_divergence"] for st in stats) >= 2 * 5
    assert m.tile_context(2).n == 0 and len(m.download()["ids"]) == N
    ctx = single_context(6, y.default_params(fixed_iterations=(2, 2)))
    a, b = m.download(), ctx.download()
    oa, ob = np.argsort(a["ids"], kind="stable"), np.argsort(b["ids"], kind="stable")
    for f in ("pos", "vel"):
        assert np.array_equal(bits(a[f][oa]), bits(b[f][ob])), f
    ctx.close()
    m.close()


def test_every_point_is_answered_exactly_once(run40):
    """through the seam the multi call is built on: the records of all tiles together hold every index once"""
    world, m, K, snaps = run40
    pts = snaps[-1]["pts"]
    L, n = m.L, len(pts)
    seen = np.zeros(n, np.int64)
    for k in range(world):
        t = m.tile_context(k)
        assert L.sphx_tile_sample_points(t.h, pts.ctypes.data, n, y.KERNEL_WENDLAND_C2, _lib.SAMPLE_FIELD_BITS["count"]) == 0, L.sphx_last_error(t.h)
    for k in range(world):
        rec = np.zeros((n, 6), np.uint32)
        got = C.c_uint32()
        assert L.sphx_tile_sample_points_fetch(m.tile_context(k).h, rec.ctypes.data, n, C.byref(got)) == 0
        np.add.at(seen, rec[:got.value, 0], 1)
        assert not rec[:got.value, 1:5].any()  # (fields that were not asked for are stored as zero)
    assert (seen == 1).all()
    # a 65-point set: one full wavefront plus one lane
    few = m.sample(pts[:65], tiles=True)
    for f in few:
        assert np.array_equal(bits(few[f]), bits(snaps[-1]["full"][y.KERNEL_WENDLAND_C2][f][:65])), f


def test_the_plain_calls_still_refuse_a_tile(run40):
    world, m, K, snaps = run40
    msg = refused(_lib.ERR_INVALID_ARGUMENT, m.tile_context(0).sample, snaps[0]["pts"][:4])
    assert "tile context" in msg


# ---- 5. lattice equals points ------------------------------------------------------------------------------------------------------------------
def test_lattice_equals_points(run40):
    world, m, K, snaps = run40
    s = snaps[-1]
    for kind in KINDS:
        g, p = s["grid"][kind], s["full"][kind]
        n_lat = LATTICE[4] * LATTICE[5]
        for f in g:
            assert np.array_equal(bits(g[f]).reshape(n_lat, -1), bits(p[f][:n_lat]).reshape(n_lat, -1)), (world, kind, f)
    cases = [((F(0.2), F(0.9)), (F(0.0071), F(0.0069)), (33, 29)),      # dx below a cell
             ((F(-0.3), F(-0.2)), (F(0.057), F(0.083)), (31, 37)),      # above a cell
             ((F(0.31), F(0.4)), (F(0.01), F(0.013)), (150, 1)),        # nx == 1
             ((F(0.05), F(1.1)), (F(0.009), F(0.01)), (1, 90)),         # ny == 1
             ((F(0.12), F(0.72)), (F(0.004), F(0.004)), (17, 17)),      # one full workgroup tile plus an edge, wholly inside one tile
             ((F(-150.0), F(-140.0)), (F(31.0), F(29.0)), (55, 53))]    # larger than the domain on every side
    for origin, spacing, shape in cases:
        g = m.sample_grid(origin, spacing, shape, tiles=True)
        pts = sr.lattice_points(origin[0], origin[1], spacing[0], spacing[1], shape[1], shape[0])
        p = m.sample(pts, tiles=True)
        for f in g:
            assert g[f].shape[:2] == tuple(shape)
            assert np.array_equal(bits(g[f]).reshape(len(pts), -1), bits(p[f]).reshape(len(pts), -1)), (world, origin, f)
        assert np.array_equal(g["tile"].ravel(), owner_of(K, s["rects"], pts))
    inside = m.sample_grid((F(0.12), F(0.72)), (F(0.004), F(0.004)), (17, 17), tiles=True)
    assert len(np.unique(inside["tile"])) == 1 and inside["count"].min() > 0


# ---- 2. against a single context in tiling-invariant mode ----------------------------------------------------------------------------------
def single_context(steps, params):
    ctx = y.SphxContext(params)
    ctx.set_tiling_invariant(True)
    ctx.set_boundary(BOUNDARY)
    ctx.upload(POS)
    if steps == 0:  # (a single context computes the densities of uploaded positions on request)
        ctx.update_neighborhood()
        ctx.update_densities()
    timer = y.TimeManager()
    for _ in range(steps):
        vmax = ctx.step_begin(timer.simulation_step(), timer.law(DIAM))
        ctx.step_finish(y.duration_as_secs_f32(timer.update_simulation_step(DIAM, vmax)))
    return ctx


GAUGES = ((0.15, 0.3, 0.45, 0.58, 1.5), 0.5, 1.9, 0.004)


@pytest.mark.parametrize("tiling", TILINGS, ids=TILING_IDS)
def test_tiling_invariant_mode_equals_the_single_context(tiling):
    """set up as tests/test_gpu_multi.py sets the mode up: fixed 2 + 2 iterations, cell mates ordered by id on both sides"""
    world, strips = tiling
    fixed = (2, 2)
    m = new_multi(world, strips, params=y.default_params(fixed_iterations=fixed), halo=16, invariant=True)
    m.upload(POS)
    timer = y.TimeManager()
    for steps in (0, 40):
        if steps:
            m.steps(timer, steps)
        ctx = single_context(steps, y.default_params(fixed_iterations=fixed))
        pts = point_set(m.tile_rects(), tile_states(m))
        for kind in KINDS:
            assert_bits(m.sample(pts, kind), ctx.sample(pts, kind), "%d tiles, %d steps, kind %d" % (world, steps, kind))
            g = m.sample_grid(LATTICE[:2], LATTICE[2:4], (LATTICE[5], LATTICE[4]), kind)
            assert_bits(g, ctx.sample_grid(LATTICE[:2], LATTICE[2:4], (LATTICE[5], LATTICE[4]), kind), "%d tiles, %d steps, kind %d, lattice" % (world, steps, kind))
        a, b = y.gauge_elevation(m, *GAUGES), y.gauge_elevation(ctx, *GAUGES)
        assert np.array_equal(a, b, equal_nan=True) and np.isfinite(a[:4]).all() and np.isnan(a[4]), (a, b)
        ctx.close()
    m.close()


# ---- 3. spent band ----------------------------------------------------------------------------------------------------------------------------
def test_a_spent_ghost_band_is_refreshed_by_the_query():
    """fixed halo of 7 cells, 2 density and 3 divergence iterations: from the second step on the divergence loop (a warm start and three
    iterations: 1 + 2 * 3 rings) ends with valid = 0.  The query then makes the exchange the next step_begin owes."""
    fixed = (2, 3)
    m = new_multi(2, None, params=y.default_params(fixed_iterations=fixed), halo=7, fixed_halo=True, invariant=True)
    m.upload(POS)
    timer = y.TimeManager()
    m.steps(timer, 6)
    rings = m.ghost_rings()
    assert rings["valid"] < 1, rings  # the precondition of this test: the band is spent at the query
    ctx = single_context(6, y.default_params(fixed_iterations=fixed))
    pts = point_set(m.tile_rects(), tile_states(m))
    before = m.info()["exchanges"]
    got = m.sample(pts)
    assert m.info()["exchanges"] == before + 1
    after = m.ghost_rings()
    assert after["valid"] == 7 and after["avalid"] == 6, after
    assert_bits(got, ctx.sample(pts), "spent band, points")
    assert_bits(m.sample_grid(LATTICE[:2], LATTICE[2:4], (LATTICE[5], LATTICE[4])), ctx.sample_grid(LATTICE[:2], LATTICE[2:4], (LATTICE[5], LATTICE[4])),
                "spent band, lattice")
    assert m.info()["exchanges"] == before + 1  # (the second query found a full band)
    m.step_begin(timer.simulation_step())
    assert m.info()["exchanges"] == before + 1  # ... and so does the step: the exchange it owed has happened
    ctx.close()
    m.close()


# ---- 4. no trace in the run -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 4], ids=["2 strips", "2x2"])
def test_queries_leave_no_trace_in_the_run(world):
    pts = np.ascontiguousarray(np.concatenate([sr.lattice_points(*LATTICE)[::3], POS[::9]]), F)
    runs = []
    for sampling in (False, True):
        m = new_multi(world)
        m.upload(POS)
        timer = y.TimeManager()
        stats = []
        for _ in range(40):
            stats.append(m.step(timer))
            if sampling:
                m.sample(pts)
                m.sample_grid((F(0.0), F(0.6)), (F(0.011), F(0.013)), (40, 50), fields=("fraction", "velocity"))
        d = m.download()
        order = np.argsort(d["ids"], kind="stable")
        digest = m.state_digest()
        m.step_begin(timer.simulation_step())
        runs.append(dict(stats=stats, d={k: v[order] for k, v in d.items()}, digest=digest, exchanges=m.info()["exchanges"], rebalances=m.info()["rebalances"]))
        m.close()
    a, b = runs
    for k in range(40):
        assert set(STEP_FIELDS) - {"reserved"} <= set(a["stats"][k]) and a["stats"][k] == b["stats"][k], (k, a["stats"][k], b["stats"][k])
    for f in a["d"]:
        assert np.array_equal(bits(a["d"][f]), bits(b["d"][f])), f
    assert a["digest"] == b["digest"] and a["exchanges"] == b["exchanges"] and a["rebalances"] == b["rebalances"] >= 1


# ---- 6. refusals and no-ops ----------------------------------------------------------------------------------------------------------------
def test_refusals_and_no_ops():
    bad, not_ready = _lib.ERR_INVALID_ARGUMENT, _lib.ERR_NOT_READY
    pts = np.ascontiguousarray(POS[:10], F)
    m = new_multi(2)
    L = m.L
    buf = np.zeros(64, F)
    o = _lib.SphxMultiSampleOut(buf.ctypes.data, None, None, None, None)

    def points(n=10, kind=0, flags=0, out=o, xy=pts.ctypes.data):
        return L.sphx_multi_sample_points(m.h, xy, n, kind, flags, C.byref(out) if out is not None else None), L.sphx_multi_last_error(m.h).decode()

    def grid(x0=0.0, y0=0.0, dx=0.1, dy=0.1, nx=4, ny=4, kind=0, flags=0, out=o):
        return L.sphx_multi_sample_grid(m.h, x0, y0, dx, dy, nx, ny, kind, flags, C.byref(out) if out is not None else None), L.sphx_multi_last_error(m.h).decode()

    # arguments first (they name the argument), before the first upload too
    for call in (points, grid):
        rc, msg = call(out=None)
        assert rc == bad and "out is NULL" in msg
        rc, msg = call(out=_lib.SphxMultiSampleOut())
        assert rc == bad and "requests no output" in msg
        rc, msg = call(out=_lib.SphxMultiSampleOut(None, None, None, None, buf.ctypes.data))  # tile alone is none of the four fields
        assert rc == bad and "requests no output" in msg
        rc, msg = call(kind=3)
        assert rc == bad and "kernel_kind" in msg
        rc, msg = call(flags=1)
        assert rc == bad and "flags" in msg
    rc, msg = points(xy=None)
    assert rc == bad and "xy is NULL" in msg
    for kw, word in ((dict(x0=float("nan")), "x0 / y0"), (dict(y0=float("inf")), "x0 / y0"), (dict(dx=0.0), "dx"), (dict(dx=float("inf")), "dx"),
                     (dict(dy=-1.0), "dy"), (dict(dy=float("nan")), "dy"), (dict(nx=1 << 16, ny=1 << 15), "nx * ny")):
        rc, msg = grid(**kw)
        assert rc == bad and word in msg, (kw, msg)
    # no-ops once the arguments pass, whatever the state
    assert points(n=0)[0] == 0 and points(n=0, xy=None)[0] == 0 and grid(nx=0)[0] == 0 and grid(ny=0)[0] == 0
    # before the first upload
    assert points()[0] == not_ready and "upload" in points()[1] and grid()[0] == not_ready
    refused(not_ready, m.tile_rects)
    m.upload(POS)
    assert points()[0] == 0 and grid()[0] == 0
    assert set(m.ghost_rings()) == {"valid", "kvalid", "avalid"} and m.tile_rects().shape == (2, 4)
    # between step_begin and step_finish
    timer = y.TimeManager()
    m.step_begin(timer.simulation_step())
    rc, msg = points()
    assert rc == not_ready and "step" in msg and grid()[0] == not_ready
    m.step_finish(F(0.001))
    assert points()[0] == 0
    # a multi that a failed state load left broken: one payload word corrupted, the host checks pass, the device digest does not
    blob = m.save_state()
    forged = bytearray(blob)
    forged[mref.parse_part(blob)["table"]["velocities"][0] + 8 * (N // 2)] ^= 0x10
    refused(bad, m.load_state, bytes(forged))
    rc, msg = points()
    assert rc == not_ready and "did not complete" in msg and grid()[0] == not_ready
    m.load_state(blob)  # ... and a load puts it right
    assert points()[0] == 0 and grid()[0] == 0
    # the seam: a plain context is refused, a tile context accepted
    ctx = y.SphxContext()
    win = (C.c_uint32 * 4)()
    assert L.sphx_tile_sample_points(ctx.h, pts.ctypes.data, 10, 0, 1) == bad and "not a tile context" in L.sphx_last_error(ctx.h).decode()
    assert L.sphx_tile_sample_window(ctx.h, 0.0, 0.0, 0.1, 0.1, 4, 4, 0, 1, win) == bad
    ctx.close()
    t = m.tile_context(0)
    assert L.sphx_tile_sample_points(t.h, pts.ctypes.data, 10, 0, 0) == bad and L.sphx_tile_sample_points(t.h, pts.ctypes.data, 10, 0, 16) == bad
    assert L.sphx_tile_sample_points(t.h, pts.ctypes.data, 10, 7, 1) == bad
    m.close()
    # more than 64 tiles cannot be made on one device here; a one-tile multi has infinite rings
    one = new_multi(1)
    one.upload(POS)
    assert one.ghost_rings()["valid"] == float("inf") and one.tile_rects().tolist() == [[0, 65536, 0, 65536]]
    one.close()


def test_solver_object_reaches_the_tiled_sampling():
    w = y.FluidParticleWorld()
    w.reset_fluid(1.0)
    s = y.DFSPHMultiSolver(w, [0, 0])
    t = y.TimeManager()
    pts = np.ascontiguousarray(POS[::13], F)
    assert "before the first" in refused(_lib.ERR_NOT_READY, s.sample, pts)  # (the solver uploads with its first step)
    s.simulation_steps(w, t, 5, sync_world=False)
    m = s.multi()
    K = consts_of(m, y.default_params())  # (a borrowed multi carries no params: the solver object runs the defaults)
    states, rects = tile_states(m), m.tile_rects()
    got = s.sample(pts, tiles=True)
    owner = owner_of(K, rects, pts)
    assert np.array_equal(got["tile"], owner) and len(np.unique(owner)) == 2
    assert_bits(got, reference(K, states, owner, pts, y.KERNEL_WENDLAND_C2), "the solver object's tiles")
    g = s.sample_grid((F(0.1), F(0.7)), F(0.02), (17, 17), fields=("fraction",))
    assert sorted(g) == ["fraction"] and g["fraction"].shape == (17, 17)
    assert np.array_equal(bits(g["fraction"]).ravel(), bits(s.sample(sr.lattice_points(F(0.1), F(0.7), F(0.02), F(0.02), 17, 17), fields="fraction")["fraction"]))
    e = y.gauge_elevation(s, (0.3,), 0.5, 1.9, 0.004)
    assert np.array_equal(e, y.gauge_elevation(m, (0.3,), 0.5, 1.9, 0.004)) and 1.5 < e[0] < 1.75
    s.close()


# ---- 7. one process per tile ----------------------------------------------------------------------------------------------------------------
def test_rank_mode_parts_fold_to_the_in_process_run(tmp_path):
    """Two processes over gloo (the halo records) and the shared segment (the scalars), both on device 0.  Each rank's part has zeros
    and tile -1 where the other rank answers; the parts, folded with sample_merge, are the bytes of the in-process devices=[0, 0] run."""
    steps = 12
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1", "--master-port", "29567",
           os.path.join(HERE, "sample_multi_rank_worker.py"), str(tmp_path), str(steps)]
    p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    r = [np.load(tmp_path / f"rank{k}.npz") for k in range(2)]
    pts = r[0]["pts"]
    assert np.array_equal(bits(pts), bits(r[1]["pts"]))
    for k in range(2):  # both calls, on both ranks, refused out->tile == NULL (the worker also checked the message and that no exchange ran)
        assert r[k]["refused_without_tile"].tolist() == [_lib.ERR_INVALID_ARGUMENT] * 2
    m = new_multi(2)
    m.upload(POS)
    m.steps(y.TimeManager(), steps)
    lat = tuple(r[0]["lattice"].tolist())
    for prefix, want in (("points_", m.sample(pts, tiles=True)), ("grid_", m.sample_grid(lat[:2], lat[2:4], (int(lat[5]), int(lat[4])), tiles=True))):
        parts = [{f: (r[k][prefix + f].view(F) if f in ("density", "fraction", "velocity") else r[k][prefix + f]) for f in sr.FIELDS + ("tile",)} for k in range(2)]
        for k, part in enumerate(parts):
            mine = part["tile"] == k
            assert np.array_equal(mine, want["tile"] == k) and (part["tile"][~mine] == -1).all()
            for f in sr.FIELDS:
                assert not bits(part[f])[~mine].any(), (prefix, k, f)  # zeros where the other rank answers
            assert mine.any() and (~mine).any()
        got = y.sample_merge(parts)
        for f in want:
            assert np.array_equal(bits(got[f]), bits(want[f])), (prefix, f)
    m.close()
