"""Neighbour queries of a tiled run on the device (include/sphx.h, "neighbour queries of a tiled run"): sphx_multi_query_radius,
sphx_multi_select and the fold of the ranks' parts.  The expected values never come from the calls under test: they are the float32
restatement of the query contract (tests/query_reference.py) over the answering tile's own downloads, folded by
tests/query_multi_reference.py, a search over all particles of MultiSolver.download(), or the single context in tiling-invariant mode.
Everything is compared as bits.  The scenes are the dam break of tests/util.py at scale 1.0 (4 050 particles, every tile on device 0)
with small halos and a re-partition every 4 steps, so that ghosts, migration and moving cuts really happen.  The host side (the fold) is
checked without a GPU in tests/test_query_multi_host.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import query_multi_reference as qm
import query_reference as qr
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
SENTINEL = 0xA5A5A5A5
# the fluid lies in the cell columns 5005 .. 5029 at t = 0: the last of these three strips holds the right-hand walls and no fluid
THREE_STRIPS = (0, [0, 5017, 5060, 65536])
# (tiles, explicit strips, halo): the last one runs with a 3-cell halo, the smallest band a solver iteration (two rings) fits in
TILINGS = [(1, None, 10), (2, None, 10), (4, None, 10), (3, THREE_STRIPS, 10), (2, None, 3)]
TILING_IDS = ["one tile", "2 strips", "2x2", "3 strips, one without fluid", "2 strips, halo 3"]
STATES = (0, 1, 12)  # steps: after the upload, after one step, after 12 (three re-partitions)
# h, 0.9 h and 0.5 h; and one whose square underflows to zero in fp32: only d2 == 0 is accepted
RADII = (H, F(F(0.9) * H), F(F(0.5) * H), F(1e-30))
LATTICE = (F(-0.07), F(-0.09), F(0.0413), F(0.0391), 57, 71)
bits = qm.bits


def refused(code, fn, *args, **kw):
    with pytest.raises(y.SphxError) as e:
        fn(*args, **kw)
    assert e.value.code == code, str(e.value)
    return str(e.value)


def new_multi(world, strips=None, halo=10, params=None, rebalance_every=4, invariant=False, boundary=BOUNDARY, **kw):
    m = MultiSolver(params if params is not None else y.default_params(), devices=[0] * world, halo=halo, rebalance_every=rebalance_every, **kw)
    if invariant:
        m.set_tiling_invariant(True)
    if strips is not None:
        m.set_strips(*strips)
    m.set_boundary(boundary)
    return m


def consts_of(m, params=None):
    return sr.Constants(params if params is not None else m.params, m.tile_context(0).constants())


def cell_centre(c):
    return (F(-100.0) + (F(c) + F(0.5)) * H).astype(F)


def point_set(rects, states, seed=11):
    """about 3 000 points: a thinned lattice over the scene; 300 points exactly on particles; for every cut the last owned cell column /
    row on one side and the first on the other, also shifted by +-h (their neighbours are mostly ghosts); a run of 600 consecutive points
    that alternates across the first cut (mixed ownership inside every wavefront); points beside the right wall (the fluid-less strip);
    far-away, infinite and NaN points"""
    rng = np.random.default_rng(seed)
    pos = np.concatenate([s["pos"][(s["ids"] >> 31) == 1] for s in states])
    pts = [sr.lattice_points(*LATTICE)[::5], pos[rng.choice(len(pos), 300, replace=False)]]
    ys = (F(0.55) + np.arange(48, dtype=F) * F(0.0257)).astype(F)  # through the fluid column and above it
    xs = (F(0.05) + np.arange(32, dtype=F) * F(0.0213)).astype(F)
    cuts = []
    for x0, x1, y0, y1 in rects.tolist():
        cuts += [(0, c) for c in (x0, x1) if 0 < c < 65536] + [(1, c) for c in (y0, y1) if 0 < c < 65536]
    cuts = sorted(set(cuts))
    for axis, c in cuts:
        for line in (c - 1, c):
            for shift in (F(0.0), H, -H):
                fixed = np.full(len(ys if axis == 0 else xs), cell_centre(line) + shift, F)
                pts.append(np.stack([fixed, ys], -1) if axis == 0 else np.stack([xs, fixed], -1))
    if cuts:
        axis, c = cuts[0]
        k = np.arange(600)
        across = np.where(k % 2 == 0, cell_centre(c - 1), cell_centre(c)).astype(F)
        along = ((F(0.52) if axis == 0 else F(0.02)) + (k // 2).astype(F) * F(0.0031)).astype(F)
        pts.append(np.stack([across, along], -1) if axis == 0 else np.stack([along, across], -1))
    else:
        pts.append(sr.lattice_points(*LATTICE)[1::3])  # (one tile: no cut to probe)
    wall = BOUNDARY[BOUNDARY[:, 0] > F(1.3)]
    pts.append((wall[rng.choice(len(wall), 200, replace=False)] + rng.normal(0, 0.007, (200, 2))).astype(F))
    pts.append(np.array([[1e6, 1e6], [-1e30, 0.5], [np.nan, 0.5], [0.5, np.nan], [np.inf, 0.5], [-np.inf, -np.inf], [-200.0, -200.0],
                         [3.4e38, -3.4e38]], F))
    return np.ascontiguousarray(np.concatenate(pts), F)


def raw_query(m, pts, radius, cap, flags=0, lists=True, pad=16):
    """the C call with sentinel-filled outputs `pad` entries longer than cap -> (rc, arrays)"""
    n = len(pts)
    a = dict(offsets=np.full(n + 1, SENTINEL, np.uint64), count=np.full(1, SENTINEL, np.uint64), nearest_id=np.full(n, SENTINEL, np.uint32),
             nearest_slot=np.full(n, SENTINEL, np.uint32), nearest_dist_sq=np.full(n, SENTINEL, np.uint32).view(F), tile=np.full(n, -9, np.int32))
    if lists:
        a.update(id=np.full(cap + pad, SENTINEL, np.uint32), slot=np.full(cap + pad, SENTINEL, np.uint32),
                 dist_sq=np.full(cap + pad, SENTINEL, np.uint32).view(F))
    o = _lib.SphxMultiQueryOut(**{k: v.ctypes.data for k, v in a.items()})
    rc = m.L.sphx_multi_query_radius(m.h, pts.ctypes.data, n, float(radius), cap, flags, C.byref(o))
    return rc, a


def snapshot(m, what):
    """everything the device says about one state, taken while the multi is in it"""
    rects, states = m.tile_rects(), qm.tile_states(m)
    pts = point_set(rects, states)
    s = dict(what=what, rects=rects, states=states, pts=pts, whole=m.download(), exchanges=m.info()["exchanges"], got={})
    for boundary in (False, True):
        for r in RADII:
            s["got"][(boundary, float(r))] = m.query(pts, r, boundary=boundary, tiles=True)
    s["again"] = m.query(pts, H, tiles=True)
    s["exchanges_after"] = m.info()["exchanges"]
    return s


@pytest.fixture(scope="module", params=TILINGS, ids=TILING_IDS)
def run12(request):
    """default mode: (world, multi, constants, the snapshots after the upload, after 1 step and after 12 with a re-partition every 4)"""
    world, strips, halo = request.param
    m = new_multi(world, strips, halo)
    m.upload(POS)
    timer = y.TimeManager()
    snaps, done = [], 0
    for steps in STATES:
        if steps > done:
            m.steps(timer, steps - done)
            done = steps
        snaps.append(snapshot(m, "after %d steps" % steps))
    yield world, m, consts_of(m), snaps
    m.close()


# ---- 1. against the answering tile; 3. against a search over the whole run; 4. slot; 6. determinism -------------------------------------------
def test_bit_identical_to_the_answering_tiles_own_arrays(run12):
    world, m, K, snaps = run12
    for s in snaps:
        what = "%d tiles, %s" % (world, s["what"])
        pts, states = s["pts"], s["states"]
        assert 2000 <= len(pts) <= 4500 and len(states) == world
        owner = qm.owner_of(K, s["rects"], pts)
        assert np.bincount(owner, minlength=world).max() > 256  # (the carry across the workgroups of the selection)
        if world > 1:
            assert len(np.unique(owner)) == world, what + ": the point set does not reach every tile"
            assert (owner[:-1] != owner[1:]).sum() >= 599, what + ": no run of points that alternates across a cut"
        maps = qm.boundary_maps(states, BOUNDARY)
        for (boundary, r), got in s["got"].items():
            ref = qm.reference(K, states, maps, owner, pts, F(r), boundary)
            qm.assert_same(got, ref, "%s, radius %g, boundary %d" % (what, r, boundary))
            # far and non-finite points: empty lists, answered by the tile of their saturated cell
            assert not np.diff(got["offsets"].astype(np.int64))[-8:].any() and (got["nearest_id"][-8:] == qm.NONE).all()
            # 4. slot: the answering tile's download holds that id there, and the position whose d2 is dist_sq
            qi = np.repeat(np.arange(len(pts)), np.diff(got["offsets"].astype(np.int64)))
            for t, st in enumerate(states):
                e = np.nonzero(got["tile"][qi] == t)[0]
                p = (st["boundary"] if boundary else st["pos"])[got["slot"][e]]
                ids = maps[t][st["boundary_ids"][got["slot"][e]]] if boundary else st["ids"][got["slot"][e]] & np.uint32(0x7FFFFFFF)
                assert np.array_equal(ids, got["id"][e]), what
                dx, dy = (p[:, 0] - pts[qi[e], 0]).astype(F), (p[:, 1] - pts[qi[e], 1]).astype(F)
                assert np.array_equal(bits(((dx * dx).astype(F) + (dy * dy).astype(F)).astype(F)), bits(got["dist_sq"][e])), what
            if boundary:
                assert got["count"] == 0 or got["id"].max() < len(BOUNDARY)
        full = s["got"][(False, float(H))]
        # the points meet the fluid (300 of them sit on particles 0.01 apart: at least 8 within h each), and the particles they sit on
        assert full["count"] > 2400 and (full["dist_sq"] == 0).sum() >= 300
        tiny = s["got"][(False, float(RADII[3]))]
        assert tiny["count"] >= 300 and not tiny["dist_sq"].any()  # r2 underflows: only d2 == 0 is accepted
        assert s["got"][(True, float(H))]["count"] >= 200  # (200 points lie within a cell of the right wall)
        # 3. at 0.9 h and 0.5 h: every particle of the whole run within the radius, whatever the tiling
        for r in RADII[1:3]:
            brute = qr.brute32(dict(pos=s["whole"]["pos"], ids=s["whole"]["ids"], boundary=BOUNDARY), pts, r)
            assert np.array_equal(qm.point_id_pairs(s["got"][(False, float(r))]), qm.point_id_pairs(brute)), "%s: radius %g" % (what, r)
            brute = qr.brute32(dict(pos=s["whole"]["pos"], boundary=BOUNDARY), pts, r, boundary=True)
            assert np.array_equal(qm.point_id_pairs(s["got"][(True, float(r))]), qm.point_id_pairs(brute)), "%s: radius %g, boundary" % (what, r)
        # 6. two calls return the same bytes; no call exchanged anything
        for f, a in s["again"].items():
            assert np.array_equal(bits(np.asarray(a)), bits(np.asarray(full[f]))), f
        assert s["exchanges_after"] == s["exchanges"]


def test_the_fluid_less_strip_answers(run12):
    """the strip that holds walls and no fluid: empty lists over the fluid, its static grid with boundary=True"""
    world, m, K, snaps = run12
    if world != 3:
        return
    s = snaps[0]
    assert len(s["states"][2]["pos"]) == 0 and len(s["states"][2]["boundary"]) > 0
    there = qm.owner_of(K, s["rects"], s["pts"]) == 2
    assert there.sum() >= 200
    fluid, walls = s["got"][(False, float(H))], s["got"][(True, float(H))]
    assert not np.diff(fluid["offsets"].astype(np.int64))[there].any() and (fluid["tile"][there] == 2).all()
    assert (np.diff(walls["offsets"].astype(np.int64))[there] > 0).sum() >= 100


# ---- 5. capacity ---------------------------------------------------------------------------------------------------------------------------
def test_capacity_and_guard_words(run12):
    world, m, K, snaps = run12
    s = snaps[-1]
    pts = s["pts"]
    for boundary in (False, True):
        full = s["got"][(boundary, float(H))]
        i = int(np.argmax(np.diff(full["offsets"].astype(np.int64)) >= 3))
        for cap in (int(full["offsets"][i]) + 1, 0, full["count"] - 1, full["count"], full["count"] + 5):
            rc, a = raw_query(m, pts, H, cap, _lib.QUERY_BOUNDARY if boundary else 0)
            n = min(cap, full["count"])
            assert rc == 0 and a["count"][0] == full["count"] and np.array_equal(a["offsets"], full["offsets"]), (cap, boundary)
            for f in ("id", "slot", "dist_sq"):
                assert np.array_equal(bits(a[f][:n]), bits(full[f][:n])), (f, cap)
                assert (bits(a[f][n:]) == SENTINEL).all(), (f, cap)  # nothing at or behind the capacity, nothing behind the total
            for f in ("nearest_id", "nearest_slot", "nearest_dist_sq", "tile"):
                assert np.array_equal(bits(a[f]), bits(full[f])), (f, cap)
    # offsets and nearest alone: one walk, no entry array
    rc, a = raw_query(m, pts, H, 1 << 40, lists=False)
    full = s["got"][(False, float(H))]
    assert rc == 0 and a["count"][0] == full["count"] and np.array_equal(a["offsets"], full["offsets"]) and np.array_equal(a["nearest_id"], full["nearest_id"])
    part = m.query(pts, H, cap=1234)
    assert part["count"] == full["count"] and len(part["id"]) == 1234 and np.array_equal(part["id"], full["id"][:1234])
    assert sorted(m.query(pts[:10], H, lists=False, nearest=False)) == ["count", "offsets"]


# ---- 2. against a single context in tiling-invariant mode -------------------------------------------------------------------------------------
def single_context(steps, params):
    ctx = y.SphxContext(params)
    ctx.set_tiling_invariant(True)
    ctx.set_boundary(BOUNDARY)
    ctx.upload(POS)
    if steps == 0:
        ctx.update_neighborhood()
        ctx.update_densities()
    timer = y.TimeManager()
    for _ in range(steps):
        vmax = ctx.step_begin(timer.simulation_step(), timer.law(DIAM))
        ctx.step_finish(y.duration_as_secs_f32(timer.update_simulation_step(DIAM, vmax)))
    return ctx


@pytest.mark.parametrize("tiling", TILINGS[:4], ids=TILING_IDS[:4])
def test_tiling_invariant_mode_equals_the_single_context(tiling):
    """fixed 2 + 2 iterations, cell mates ordered by id on both sides: offsets, id, dist_sq, nearest_id, nearest_dist_sq and count are the
    single context's bytes (slot is tile-local by definition)"""
    world, strips, _ = tiling
    fixed = (2, 2)
    m = new_multi(world, strips, 16, params=y.default_params(fixed_iterations=fixed), invariant=True)
    m.upload(POS)
    timer = y.TimeManager()
    done = 0
    for steps in (0, 12):
        if steps > done:
            m.steps(timer, steps - done)
            done = steps
        ctx = single_context(steps, y.default_params(fixed_iterations=fixed))
        pts = point_set(m.tile_rects(), qm.tile_states(m))
        d, bid = ctx.download(), ctx.download_boundary()[1]
        for boundary in (False, True):
            ids = bid if boundary else d["ids"]
            for r in RADII:
                got, one = m.query(pts, r, boundary=boundary), ctx.query(pts, r, boundary=boundary)
                what = "%d tiles, %d steps, radius %g, boundary %d" % (world, steps, r, boundary)
                assert got["count"] == one["count"] and np.array_equal(got["offsets"], one["offsets"]), what
                assert np.array_equal(got["id"], one["id"]) and np.array_equal(bits(got["dist_sq"]), bits(one["dist_sq"])), what
                near = np.where(one["nearest"] != qm.NONE, ids[np.minimum(one["nearest"], len(ids) - 1)], qm.NONE) if len(ids) else one["nearest"]
                assert np.array_equal(got["nearest_id"], near) and np.array_equal(bits(got["nearest_dist_sq"]), bits(one["nearest_dist_sq"])), what
        ctx.close()
    m.close()


# ---- 7. no trace in the run ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 4], ids=["2 strips", "2x2"])
def test_queries_and_selects_leave_no_trace_in_the_run(world):
    pts = np.ascontiguousarray(np.concatenate([sr.lattice_points(*LATTICE)[::3], POS[::9]]), F)
    runs = []
    for asking in (False, True):
        m = new_multi(world)
        m.upload(POS)
        timer = y.TimeManager()
        stats = []
        for k in range(16):
            stats.append(m.step(timer))
            if asking:
                m.query(pts, H)
                m.query(pts, H, boundary=True, lists=False)
                m.select([(0.2, 0.5, 0.4, 1.5)], outside=bool(k % 2))
        runs.append(dict(stats=stats, digest=m.state_digest(), exchanges=m.info()["exchanges"], rebalances=m.info()["rebalances"]))
        m.close()
    a, b = runs
    assert a["stats"] == b["stats"] and a["digest"] == b["digest"]
    assert a["exchanges"] == b["exchanges"] > 0 and a["rebalances"] == b["rebalances"]


# ---- dense cell: the direct-store path, the entries coming from ghosts on one side -----------------------------------------------------------
def test_dense_cell_beside_a_cut():
    """3 000 particles inside one cell directly beside the cut of an explicit 2-strip layout, 300 points in that cell and 300 in the
    neighbouring cell across the cut at radius h: ~900 000 entries per side, more than 4 096 per workgroup (the direct stores), on one
    side all of them from ghosts.  Also 1, 2 and 257 points, as test_dense_cell of tests/test_gpu_query.py."""
    params = y.default_params()
    K0 = sr.Constants(params)
    h = K0.h
    rng = np.random.default_rng(3)
    cell = sr.cells_of(K0, np.array([[0.5, 0.5]], F))[0]
    corner = (np.floor((np.array([0.5, 0.5], F) - K0.gmin) * K0.cell_inv) / K0.cell_inv + K0.gmin).astype(F)
    pos = (corner + (F(0.3) + F(0.4) * rng.random((3000, 2), dtype=F)) * h).astype(F)
    assert (sr.cells_of(K0, pos) == cell).all()
    m = new_multi(2, (0, [0, int(cell[0]) + 1, 65536]), 10, params=params, boundary=np.zeros((0, 2), F))  # the cut right of the dense cell
    m.upload(pos)
    K = consts_of(m)
    states, rects = qm.tile_states(m), m.tile_rects()
    assert len(states[0]["pos"]) == 3000 and len(states[1]["pos"]) == 3000 and not (states[1]["ids"] >> 31).any()  # tile 1: ghosts only
    inside = (corner + (F(0.3) + F(0.4) * rng.random((300, 2), dtype=F)) * h).astype(F)
    beyond = (inside + np.array([h, 0], F)).astype(F)
    maps = qm.boundary_maps(states, np.zeros((0, 2), F))
    for pts in (np.ascontiguousarray(np.concatenate([inside, beyond])), np.ascontiguousarray(np.stack([inside, beyond], 1).reshape(-1, 2))):
        owner = qm.owner_of(K, rects, pts)
        assert (owner == 0).sum() == 300 and (owner == 1).sum() == 300
        ref = qm.reference(K, states, maps, owner, pts, h)
        assert ref["count"] > 1000000
        qm.assert_same(m.query(pts, h, tiles=True), ref, "dense cell")
        for n in (1, 2, 257):
            for sub_pts in (pts[:n], pts[-n:]):
                sub_pts = np.ascontiguousarray(sub_pts)
                sub = qm.reference(K, states, maps, qm.owner_of(K, rects, sub_pts), sub_pts, h)
                qm.assert_same(m.query(sub_pts, h, tiles=True), sub, "dense cell, %d points" % n)
                for cap in sorted({1500, max(sub["count"] - 1500, 0)}):
                    rc, a = raw_query(m, sub_pts, h, cap)
                    k = min(cap, sub["count"])
                    assert rc == 0 and a["count"][0] == sub["count"] and np.array_equal(a["offsets"], sub["offsets"])
                    for f in ("id", "slot", "dist_sq"):
                        assert np.array_equal(bits(a[f][:k]), bits(sub[f][:k])) and (bits(a[f][k:]) == SENTINEL).all(), (n, cap, f)
    assert m.query(pts, h, boundary=True)["count"] == 0
    m.close()


# ---- select -------------------------------------------------------------------------------------------------------------------------------------
def raw_select(m, rects, flags, cap, pad=16):
    arr, k = y._rect_array(rects)
    a = dict(id=np.full(cap + pad, SENTINEL, np.uint32), tile=np.full(cap + pad, -9, np.int32), slot=np.full(cap + pad, SENTINEL, np.uint32),
             count=np.full(1, SENTINEL, np.uint64))
    o = _lib.SphxMultiSelectOut(**{f: v.ctypes.data for f, v in a.items()})
    return m.L.sphx_multi_select(m.h, arr, k, flags, cap, C.byref(o)), a


def test_select(run12):
    world, m, K, snaps = run12
    s = snaps[-1]
    whole, states, rects = s["whole"], s["states"], s["rects"]
    inf = float("inf")
    scenes = [([(0.2, 0.5, 0.4, 1.5)], False), ([(0.2, 0.5, 0.4, 1.5)], True), ([], False), ([], True),
              ([(-inf, -inf, inf, inf)], False), ([(-inf, 0.8, inf, inf)], True), ([(0.4, 0.5, 0.2, 1.5), (0.3, 1.0, 0.3, 1.2)], False),
              ([(0.05 * k, 0.5 + 0.1 * k, 0.05 * k + 0.04, 0.7 + 0.1 * k) for k in range(8)], False)]
    if world > 1:
        c = int(rects[0][1] if rects[0][1] < 65536 else rects[0][3])  # the first cut: a column (strips in x, the grid) or a row
        axis = 0 if rects[0][1] < 65536 else 1
        edge = float(F(-100.0) + F(c) * H)
        lo, hi = ((edge - 0.05, -inf, edge + 0.05, inf), (edge, -inf, edge + 2 * float(H), inf)) if axis == 0 else \
                 ((-inf, edge - 0.05, inf, edge + 0.05), (-inf, edge, inf, edge + 2 * float(H)))
        scenes += [([lo], False), ([hi], False)]  # one that straddles the cut, one wholly in tile 0's ghost band
    firsts = np.concatenate(([0], np.cumsum([int((st["ids"] >> 31).sum()) for st in states])))
    for rs, outside in scenes:
        ref = qr.select32(whole["pos"], whole["ids"], rs, outside)
        got = m.select(rs, outside)
        what = "%d tiles, %r outside=%r" % (world, rs, outside)
        assert got["count"] == ref["count"] and np.array_equal(got["id"], ref["id"]), what
        assert len(np.unique(got["id"])) == len(got["id"])  # a ghost is never reported: no id twice
        for t, st in enumerate(states):
            e = got["tile"] == t
            word = st["ids"][got["slot"][e]]
            assert (word >> 31).all() and np.array_equal(word & np.uint32(0x7FFFFFFF), got["id"][e]), what  # owned there, the bit cleared here
            assert np.array_equal(np.nonzero(e)[0], np.arange(e.sum()) + np.searchsorted(ref["index"], firsts[t])), what  # tiles in rank order
        for cap in {0, 1, ref["count"] // 2, max(ref["count"] - 1, 0), ref["count"] + 3}:
            rc, a = raw_select(m, rs, _lib.SELECT_OUTSIDE if outside else 0, cap)
            n = min(cap, ref["count"])
            assert rc == 0 and a["count"][0] == ref["count"] and np.array_equal(a["id"][:n], ref["id"][:n]), (what, cap)
            assert (a["id"][n:] == SENTINEL).all() and (a["slot"][n:] == SENTINEL).all() and (a["tile"][n:] == -9).all(), (what, cap)
        by_id = m.select(rs, outside, by_id=True)
        assert np.array_equal(by_id["id"], np.sort(ref["id"]))
    if world > 1:
        assert m.select(scenes[-2][0])["count"] > 0 and len(np.unique(m.select(scenes[-2][0])["tile"])) >= 2


# ---- 8. refusals and no-ops --------------------------------------------------------------------------------------------------------------------
def test_refusals_and_no_ops():
    bad, not_ready = _lib.ERR_INVALID_ARGUMENT, _lib.ERR_NOT_READY
    pts = np.ascontiguousarray(POS[:10], F)
    m = new_multi(2)
    L = m.L
    cnt, off, ids = np.full(1, 77, np.uint64), np.full(11, 77, np.uint64), np.zeros(64, np.uint32)
    o = _lib.SphxMultiQueryOut(offsets=off.ctypes.data, id=ids.ctypes.data, count=cnt.ctypes.data)

    def query(n=10, radius=float(H), cap=64, flags=0, out=o, xy=pts.ctypes.data):
        return L.sphx_multi_query_radius(m.h, xy, n, radius, cap, flags, C.byref(out) if out is not None else None), L.sphx_multi_last_error(m.h).decode()

    scnt = np.full(1, 77, np.uint64)
    so = _lib.SphxMultiSelectOut(id=ids.ctypes.data, count=scnt.ctypes.data)
    rect = (_lib.SphxRect * 9)(*[_lib.SphxRect(0.0, 0.0, 1.0, 1.0)] * 9)

    def select(rects=rect, n=1, flags=0, cap=64, out=so):
        return L.sphx_multi_select(m.h, rects, n, flags, cap, C.byref(out) if out is not None else None), L.sphx_multi_last_error(m.h).decode()

    # arguments first (they name the argument), before the first upload too
    for kw, word in ((dict(out=None), "out is NULL"), (dict(out=_lib.SphxMultiQueryOut(offsets=off.ctypes.data)), "out->count"), (dict(xy=None), "xy is NULL"),
                     (dict(flags=1), "flags"), (dict(flags=4), "flags"), (dict(n=1 << 31), "m must be"), (dict(radius=0.0), "radius"),
                     (dict(radius=float("nan")), "radius"), (dict(radius=float(H) * 1.01), "radius"), (dict(radius=-1.0), "radius")):
        rc, msg = query(**kw)
        assert rc == bad and word in msg, (kw, msg)
    nan_rect = (_lib.SphxRect * 1)(_lib.SphxRect(0.0, float("nan"), 1.0, 1.0))
    for kw, word in ((dict(out=None), "out is NULL"), (dict(out=_lib.SphxMultiSelectOut(id=ids.ctypes.data)), "out->count"), (dict(n=9), "n_rects"),
                     (dict(rects=None), "rects is NULL"), (dict(flags=2), "flags"), (dict(rects=nan_rect), "NaN")):
        rc, msg = select(**kw)
        assert rc == bad and word in msg, (kw, msg)
    assert cnt[0] == 77 and scnt[0] == 77  # a refused call writes nothing
    # an empty point set succeeds once the arguments pass, whatever the state
    assert query(n=0)[0] == 0 and cnt[0] == 0 and off[0] == 0 and off[1] == 77 and query(n=0, xy=None)[0] == 0
    # before the first upload
    rc, msg = query()
    assert rc == not_ready and "upload" in msg
    assert select()[0] == not_ready
    m.upload(POS)
    before = m.info()["exchanges"]
    assert query()[0] == 0 and cnt[0] > 0 and select()[0] == 0 and scnt[0] > 0
    # between step_begin and step_finish
    timer = y.TimeManager()
    m.step_begin(timer.simulation_step())
    rc, msg = query()
    assert rc == not_ready and "step" in msg
    rc, msg = select()
    assert rc == not_ready and "step" in msg
    m.step_finish(F(0.001))
    assert query()[0] == 0 and select()[0] == 0
    # after an edit and after a state load: allowed without a refresh of its own
    blob = m.save_state()
    removed = m.remove([(0.0, 1.2, 0.3, 1.4)])
    assert removed > 0
    ex = m.info()["exchanges"]
    after = m.query(POS[::7], H, tiles=True)
    K = consts_of(m)
    states = qm.tile_states(m)
    qm.assert_same(after, qm.reference(K, states, qm.boundary_maps(states, BOUNDARY), qm.owner_of(K, m.tile_rects(), POS[::7]), POS[::7], H), "after a removal")
    assert m.info()["exchanges"] == ex
    first = m.append((POS[:50] + np.array([0.7, 0.0], F)).astype(F))  # (into the empty part of the tank)
    ex = m.info()["exchanges"]
    sel = m.select([(-1e9, -1e9, 1e9, 1e9)])
    assert sel["count"] == N - removed + 50 and first in sel["id"] and m.query(BOUNDARY[::7], H, boundary=True)["count"] > 0
    assert m.info()["exchanges"] == ex  # (neither call exchanges anything)
    m.load_state(blob)
    assert m.select([], outside=True)["count"] == N and m.query(POS[::7], H)["count"] > 0
    # the seam: a plain context is refused, and the plain calls keep refusing a tile
    ctx = y.SphxContext()
    part = _lib.SphxTileQueryPart()
    total = C.c_uint32()
    assert L.sphx_tile_query_radius(ctx.h, pts.ctypes.data, 10, float(H), 0, 1) == bad and "not a tile context" in L.sphx_last_error(ctx.h).decode()
    assert L.sphx_tile_query_fetch(ctx.h, 0, C.byref(part)) == bad
    assert L.sphx_tile_select(ctx.h, rect, 1, 0) == bad and "not a tile context" in L.sphx_last_error(ctx.h).decode()
    assert L.sphx_tile_select_fetch(ctx.h, 0, None, None, C.byref(total)) == bad
    ctx.close()
    t = m.tile_context(0)
    assert "tile context" in refused(bad, t.query, pts, H) and "tile context" in refused(bad, t.select, [(0, 0, 1, 1)])
    assert L.sphx_tile_query_radius(t.h, pts.ctypes.data, 10, float(H), 1, 1) == bad and L.sphx_tile_query_radius(t.h, pts.ctypes.data, 10, 1.0, 0, 1) == bad
    assert before <= m.info()["exchanges"]
    m.close()


def test_solver_object_reaches_the_tiled_queries():
    w = y.FluidParticleWorld()
    w.reset_fluid(1.0)
    s = y.DFSPHMultiSolver(w, [0, 0])
    t = y.TimeManager()
    pts = np.ascontiguousarray(POS[::13], F)
    assert "before the first" in refused(_lib.ERR_NOT_READY, s.query, pts, H)
    s.simulation_steps(w, t, 5, sync_world=False)
    m = s.multi()
    K = consts_of(m, y.default_params())
    states, rects = qm.tile_states(m), m.tile_rects()
    got = s.query(pts, H, tiles=True)
    qm.assert_same(got, qm.reference(K, states, qm.boundary_maps(states, BOUNDARY), qm.owner_of(K, rects, pts), pts, H), "the solver object's tiles")
    whole = m.download()
    assert np.array_equal(s.select([(0.2, 0.5, 0.4, 1.5)])["id"], qr.select32(whole["pos"], whole["ids"], [(0.2, 0.5, 0.4, 1.5)])["id"])
    with pytest.raises(ValueError):
        s.query(pts)  # (a borrowed multi carries no params: the radius is required)
    s.close()


# ---- one process per tile -------------------------------------------------------------------------------------------------------------------
def test_rank_mode_parts_fold_to_the_in_process_run(tmp_path):
    """Two processes over gloo (the halo records) and the shared segment (the scalars), both on device 0.  Each rank's part has empty
    ranges and tile -1 where the other rank answers; the parts, folded with query_merge, are the bytes of the in-process devices=[0, 0]
    run; the select parts concatenated are its select.  Between two steps rank 1 alone asks, with points of its own: the run goes on."""
    steps = 12
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1", "--master-port", "29581",
           os.path.join(HERE, "query_multi_rank_worker.py"), str(tmp_path), str(steps)]
    p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    r = [np.load(tmp_path / f"rank{k}.npz") for k in range(2)]
    pts = r[0]["pts"]
    assert np.array_equal(bits(pts), bits(r[1]["pts"]))
    m = new_multi(2)
    m.upload(POS)
    m.steps(y.TimeManager(), steps)
    for k in range(2):
        assert r[k]["refused_without_tile"].tolist() == [_lib.ERR_INVALID_ARGUMENT]
    # the lone query of rank 1 in the middle of the run: its own part of its own points, checked against the in-process run at that step
    for prefix, boundary in (("fluid_", False), ("walls_", True)):
        want = m.query(pts, H, boundary=boundary, tiles=True)
        parts = []
        for k in range(2):
            part = {f: r[k][prefix + f] for f in ("offsets", "tile", "id", "slot", "nearest_id", "nearest_slot")}
            part.update(dist_sq=r[k][prefix + "dist_sq"].view(F), nearest_dist_sq=r[k][prefix + "nearest_dist_sq"].view(F), count=int(r[k][prefix + "count"]))
            mine = part["tile"] == k
            assert np.array_equal(mine, want["tile"] == k) and (part["tile"][~mine] == -1).all() and mine.any() and (~mine).any()
            cnt = np.diff(part["offsets"].astype(np.int64))
            assert not cnt[~mine].any() and np.array_equal(cnt[mine], np.diff(want["offsets"].astype(np.int64))[mine])
            assert (part["nearest_id"][~mine] == qm.NONE).all() and (bits(part["nearest_dist_sq"])[~mine] == qm.INF_WORD).all()
            assert part["count"] == int(part["offsets"][-1]) == len(part["id"])
            parts.append(part)
        got = y.query_merge(parts)
        qm.assert_same(got, want, "rank mode, " + prefix)
        short = [dict(p, id=p["id"][:5], dist_sq=p["dist_sq"][:5], slot=p["slot"][:5]) for p in parts]
        assert "truncated" in refused(_lib.ERR_CAPACITY, y.query_merge, short)
    sel = m.select([(0.2, 0.5, 0.9, 1.5)], outside=True)
    for f in ("id", "tile", "slot"):
        assert np.array_equal(np.concatenate([r[k]["select_" + f] for k in range(2)]), sel[f]), f
    assert sum(int(r[k]["select_count"]) for k in range(2)) == sel["count"]
    assert int(r[1]["alone_count"]) > 0 and int(r[0]["alone_count"]) == -1  # rank 1 asked alone, between two steps
    digest = m.state_digest()
    assert all(int(r[k]["digest_" + f]) == v for k in range(2) for f, v in digest.items())  # ... and the run went on as if nobody had
    m.close()
