"""The free surface of a tiled run on the device (include/sphx.h, "free surface of a tiled run"): sphx_multi_surface_contour and the
fold of the ranks' parts.  The expected values never come from the call under test: they are tests/contour_reference.py::contour32
applied to the values MultiSolver.sample_grid returns on the same state (themselves checked against the sampling contract in
tests/test_gpu_sample_multi.py), or SphxContext.contour of a single context in tiling-invariant mode.  Everything is compared as bits.
Scenes: the 4 050-particle dam break of tests/util.py after 0 and after 12 steps (halo 10, a re-partition every 4 steps), and the
700-point spray scene of tests/test_gpu_contour.py uploaded into a multi, where the contour is everywhere — a straight cut through
the dam break meets its surface in two places only, so the conditions on how many cut cells carry segments are met by the spray.
Every tile is on device 0.  The host side (merge, apron look-up) is checked without a GPU in tests/test_contour_multi_host.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import contour_reference as cr
import sample_reference as sr
import yasph2d_amd as y
from util import dam_break, uniform_points
from yasph2d_amd import _lib
from yasph2d_amd.multi import MultiSolver

pytestmark = pytest.mark.gpu

F = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
POS, BOUNDARY = dam_break(1.0)
SPRAY = (uniform_points(700, 2500.0, 11) + F(0.3)).astype(F)  # cells 5015 .. 5041 in both axes
DIAM = F(0.01)
KINDS = (y.KERNEL_WENDLAND_C2, y.KERNEL_POLY6, y.KERNEL_SPIKY)
SENTINEL = 0xDEADBEEF
INF = 65536
STEPS = 12
SPRAY_HALO = 4
DAM_LATTICE = (F(-0.07), F(-0.09), F(0.0213), F(0.0191), 97, 113)  # over the scene rectangle, in and out of the fluid
SPRAY_LATTICE = (F(0.27), F(0.27), F(0.0119), F(0.0131), 50, 46)   # spacing 0.012 against h = 0.02
# the fluid of the dam break lies in the cell columns 5005 .. 5029 and rows 5035 .. 5084 at t = 0: the last of the three x strips holds
# walls and no fluid; the middle one of the y strips is two halo widths (of the invariant runs' halo 16) high, the least a layout allows
DAM_TILINGS = {"one tile": (1, None), "2 strips": (2, None), "3 strips, one without fluid": (3, (0, [0, 5017, 5060, INF])), "2x2": (4, None),
               "3 strips along y": (3, (1, [0, 5043, 5075, INF]))}
# the spray: explicit cuts through the cloud; the last x strip starts behind its last particle (x >= 0.84); "2x2" takes its cuts from
# the reference (grid_cuts_from).  The scene is not stepped; a halo of 4 cells lets the middle strips be 14 and 9 cells wide
SPRAY_TILINGS = {"one tile": (1, None), "2 strips": (2, (0, [0, 5028, INF])), "3 strips, one without fluid": (3, (0, [0, 5028, 5042, INF])), "2x2": (4, "grid"),
                 "3 strips along y": (3, (1, [0, 5023, 5032, INF]))}
TILING_IDS = list(DAM_TILINGS)
COMBOS = [(kind, "fraction", iso) for kind in KINDS for iso in (0.5, 0.3)] + [(kind, "density", iso) for kind in KINDS for iso in (50.37, 30.0)]


def bits(a):
    a = np.ascontiguousarray(a)
    return a if a.dtype == np.uint32 else a.view(np.uint32)


def refused(code, fn, *args, **kw):
    with pytest.raises(y.SphxError) as e:
        fn(*args, **kw)
    assert e.value.code == code, str(e.value)
    return str(e.value)


def new_multi(world, layout=None, params=None, halo=10, rebalance_every=4, invariant=False, boundary=BOUNDARY, **kw):
    m = MultiSolver(params if params is not None else y.default_params(), devices=[0] * world, halo=halo, rebalance_every=rebalance_every, **kw)
    if invariant:
        m.set_tiling_invariant(True)
    if layout is not None and layout[0] == "grid":
        m.set_grid(layout[1], layout[2])
    elif layout is not None:
        m.set_strips(*layout)
    if boundary is not None:
        m.set_boundary(boundary)
    return m


def device(m, lattice, iso=0.5, kind=y.KERNEL_WENDLAND_C2, field="fraction", **kw):
    x0, y0, dx, dy, nx, ny = lattice
    return m.contour((x0, y0), (dx, dy), (ny, nx), iso=iso, field=field, kind=kind, **kw)


def reference(m, lattice, iso=0.5, kind=y.KERNEL_WENDLAND_C2, field="fraction"):
    """contour32 over the values sample_grid returns on the same state; tile[k] = the tile that answered node 0 of cell[k]; quad [cells, 4]
    = the tiles that answered the four nodes of every cell"""
    x0, y0, dx, dy, nx, ny = lattice
    g = m.sample_grid((x0, y0), (dx, dy), (ny, nx), kind, fields=(field,), tiles=True)
    ref = cr.contour32(g[field], x0, y0, dx, dy, nx, ny, iso)
    t = g["tile"].reshape(ny, nx)
    if nx >= 2 and ny >= 2:
        ref["quad"] = np.stack([t[:-1, :-1], t[:-1, 1:], t[1:, 1:], t[1:, :-1]], -1).reshape(-1, 4)
        ref["tile"] = ref["quad"][ref["cell"], 0].astype(np.int32)
    else:
        ref["quad"], ref["tile"] = np.zeros((0, 4), np.int32), np.zeros(0, np.int32)
    return ref


def assert_same(dev, ref, what):
    assert dev["count"] == ref["count"], "%s: %d segments, the reference has %d" % (what, dev["count"], ref["count"])
    assert dev["cell"].dtype == np.uint32 and np.array_equal(dev["cell"], ref["cell"]), what + ": cells differ"
    a, b = bits(dev["segments"]), bits(ref["segments"])
    assert a.shape == b.shape and np.array_equal(a, b), "%s: %d segments differ" % (what, int((a != b).reshape(len(a), -1).any(1).sum()))
    if "tile" in dev and "tile" in ref:
        assert dev["tile"].dtype == np.int32 and np.array_equal(dev["tile"], ref["tile"]), what + ": tile is not the tile of the cell's node 0"


def check(m, lattice, iso=0.5, kind=y.KERNEL_WENDLAND_C2, field="fraction", what=""):
    ref = reference(m, lattice, iso, kind, field)
    dev = device(m, lattice, iso, kind, field, tiles=True)
    assert_same(dev, ref, "%s %s iso %g kind %d" % (what, field, iso, kind))
    return ref, dev


def interior_cuts(rects):
    """The cut lines of a layout as {name: (tiles on the low side, tiles on the high side)}: one per interior x boundary, and one per y
    boundary of each column (a 2 x 2 grid has the x cut and a y cut per column; strips have one cut between neighbours)."""
    cuts = {}
    r = rects.tolist()
    for a, (ax0, ax1, ay0, ay1) in enumerate(r):
        for b, (bx0, bx1, by0, by1) in enumerate(r):
            if ax1 == bx0 and min(ay1, by1) > max(ay0, by0):
                lo, hi = cuts.setdefault(("x", ax1), (set(), set()))
                lo.add(a), hi.add(b)
            if ay1 == by0 and (ax0, ax1) == (bx0, bx1):
                lo, hi = cuts.setdefault(("y", ay1, ax0), (set(), set()))
                lo.add(a), hi.add(b)
    return cuts


def cut_statistics(ref, rects):
    """From the reference alone: per cut line the number of segment-carrying cells with nodes answered by tiles on both sides of it; the
    number of such cells with nodes of three or more tiles; the number of saddle cells with nodes of two or more."""
    cells = np.unique(ref["cell"])
    quad = ref["quad"][cells]
    per_cut = {}
    for name, (lo, hi) in interior_cuts(rects).items():
        per_cut[name] = int((np.isin(quad, sorted(lo)).any(1) & np.isin(quad, sorted(hi)).any(1)).sum())
    n_tiles = np.array([len(set(q)) for q in quad.tolist()], np.int64).reshape(-1)
    saddle = np.isin(ref["case"][cells], (5, 10))
    return per_cut, int((n_tiles >= 3).sum()), int((saddle & (n_tiles >= 2)).sum())


def grid_cuts_from(ref, lattice):
    """The 2 x 2 cuts from the reference of the one-tile run: the segment-carrying lattice cell nearest the lattice's centre whose nodes
    fall into different grid cells in both axes; the x cut and the first column's y cut go between them, the second column is cut
    four cells higher.  Its nodes (ix, iy) and (ix, iy + 1) then belong to two tiles of the first column and (ix + 1, .) to the second."""
    x0, y0, dx, dy, nx, ny = lattice
    K = sr.Constants(y.default_params())
    cx = sr.cells_of(K, np.stack([(F(x0) + (np.arange(nx, dtype=F) * F(dx)).astype(F)).astype(F), np.zeros(nx, F)], -1))[:, 0]
    cy = sr.cells_of(K, np.stack([np.zeros(ny, F), (F(y0) + (np.arange(ny, dtype=F) * F(dy)).astype(F)).astype(F)], -1))[:, 1]
    cells = np.unique(ref["cell"])
    iy, ix = cells // (nx - 1), cells % (nx - 1)
    ok = (cx[ix] != cx[ix + 1]) & (cy[iy] != cy[iy + 1])
    assert ok.sum() >= 20, "segment-carrying cells whose nodes differ in both grid axes were meant to be common"
    ix, iy = ix[ok], iy[ok]
    k = np.argmin((ix - nx // 2) ** 2 + (iy - ny // 2) ** 2)
    xcut, ycut = int(cx[ix[k] + 1]), int(cy[iy[k] + 1])
    return ("grid", [0, xcut, INF], [[0, ycut, INF], [0, ycut + 4, INF]])


# ------------------------------------------------------------------------------------------------------------------- the scenes
def spray_multi(name, invariant=False):
    world, layout = SPRAY_TILINGS[name]
    if layout == "grid":
        one = new_multi(1, boundary=None, halo=SPRAY_HALO)
        one.upload(SPRAY)
        layout = grid_cuts_from(reference(one, SPRAY_LATTICE), SPRAY_LATTICE)
        one.close()
    m = new_multi(world, layout, boundary=None, invariant=invariant, halo=SPRAY_HALO)
    m.upload(SPRAY)
    return m


@pytest.fixture(scope="module", params=TILING_IDS)
def spray(request):
    m = spray_multi(request.param)
    yield request.param, m
    m.close()


@pytest.fixture(scope="module")
def spray3():
    """the spray in three x strips: [.., 0.56), [0.56, 0.84) and the strip without fluid"""
    m = spray_multi("3 strips, one without fluid")
    yield m
    m.close()


@pytest.fixture(scope="module")
def spray_grid():
    m = spray_multi("2x2")
    yield m
    m.close()


# ---- 1. default mode, every tiling; 3. the cuts really carry segments ------------------------------------------------------------------------
def test_spray_every_tiling_equals_the_reference(spray):
    name, m = spray
    rects = m.tile_rects()
    for kind, field, iso in COMBOS:
        ref, dev = check(m, SPRAY_LATTICE, iso, kind, field, "spray, " + name)
        assert ref["count"] > 50
        if (kind, field, iso) == (y.KERNEL_WENDLAND_C2, "fraction", 0.5):
            # non-vacuity, from the reference's own output
            pairs, three, saddles = cut_statistics(ref, rects)
            print("spray, %s: %d segments; segment-carrying cells per cut %s, with nodes of >= 3 tiles %d, saddle cells on a cut %d"
                  % (name, ref["count"], pairs, three, saddles))
            assert len(pairs) == {"one tile": 0, "2 strips": 1, "3 strips, one without fluid": 2, "2x2": 3, "3 strips along y": 2}[name]
            assert all(v >= 4 for v in pairs.values()), pairs
            if name == "2x2":  # a cell whose nodes three tiles answered, and a saddle cell on a cut
                assert three >= 1 and saddles >= 1
            # 9. the polylines of the merged segments are the reference's: closed lines, nothing dangling — watertight across the cuts
            lines, closed = cr.lines_of(ref["segments"])
            dl, dc = y.contour_lines(dev["segments"])
            assert all(closed) and cr.dangling(ref["segments"]) == (0, 0)
            assert dc == [bool(c) for c in closed] and len(dl) == len(lines) and all(np.array_equal(bits(a), bits(b)) for a, b in zip(dl, lines))
    if name == "3 strips, one without fluid":
        assert not ((m.tile_context(2).download()["ids"] >> 31) == 1).any(), "the last strip was meant to own no fluid (it holds ghosts alone)"
    # two calls on one state return the same bytes
    a, b = (device(m, SPRAY_LATTICE, tiles=True) for _ in range(2))
    assert all(a[f].tobytes() == b[f].tobytes() for f in ("segments", "cell", "tile")) and a["count"] == b["count"]


@pytest.mark.parametrize("name", TILING_IDS)
def test_dam_break_every_tiling_equals_the_reference(name):
    world, layout = DAM_TILINGS[name]
    m = new_multi(world, layout)
    m.upload(POS)
    for steps in (0, STEPS):
        if steps:
            m.steps(y.TimeManager(), steps)
        for kind, field, iso in COMBOS[::3] if steps == 0 else COMBOS:
            ref, dev = check(m, DAM_LATTICE, iso, kind, field, "dam break, %s, %d steps," % (name, steps))
            assert ref["count"] > 40
        if world > 1:
            assert len(np.unique(dev["tile"])) >= 2, "the contour was meant to be cut by several tiles"
    m.close()


# ---- 2. tiling-invariant mode -----------------------------------------------------------------------------------------------------------------
def single_context(steps, params, pos=POS, boundary=BOUNDARY):
    ctx = y.SphxContext(params)
    ctx.set_tiling_invariant(True)
    if boundary is not None:
        ctx.set_boundary(boundary)
    ctx.upload(pos)
    if steps == 0:
        ctx.update_neighborhood()
        ctx.update_densities()
    timer = y.TimeManager()
    for _ in range(steps):
        vmax = ctx.step_begin(timer.simulation_step(), timer.law(DIAM))
        ctx.step_finish(y.duration_as_secs_f32(timer.update_simulation_step(DIAM, vmax)))
    return ctx


def ctx_contour(ctx, lattice, iso, kind, field):
    x0, y0, dx, dy, nx, ny = lattice
    return ctx.contour((x0, y0), (dx, dy), (ny, nx), iso=iso, field=field, kind=kind)


@pytest.fixture(scope="module")
def singles():
    """the single context in tiling-invariant mode: the dam break after 0 and after STEPS steps, and the spray"""
    fixed = y.default_params(fixed_iterations=(2, 2))
    out = {}
    for key, ctx, lattice in ((0, single_context(0, fixed), DAM_LATTICE), (STEPS, single_context(STEPS, fixed), DAM_LATTICE),
                              ("spray", single_context(0, y.default_params(), SPRAY, None), SPRAY_LATTICE)):
        out[key] = {c: ctx_contour(ctx, lattice, c[2], c[0], c[1]) for c in COMBOS}
        ctx.close()
    return out


@pytest.mark.parametrize("name", TILING_IDS)
def test_tiling_invariant_mode_equals_the_single_context(name, singles):
    world, layout = DAM_TILINGS[name]
    m = new_multi(world, layout, params=y.default_params(fixed_iterations=(2, 2)), halo=16, invariant=True)
    m.upload(POS)
    for steps in (0, STEPS):
        if steps:
            m.steps(y.TimeManager(), steps)
        for c in COMBOS:
            want = singles[steps][c]
            assert want["count"] > 40
            assert_same(device(m, DAM_LATTICE, c[2], c[0], c[1]), want, "%s, %d steps, %s" % (name, steps, c))
    m.close()
    m = spray_multi(name, invariant=True)
    for c in COMBOS:
        assert_same(device(m, SPRAY_LATTICE, c[2], c[0], c[1]), singles["spray"][c], "spray, %s, %s" % (name, c))
    m.close()


# ---- 4. size edges ----------------------------------------------------------------------------------------------------------------------------
def windows_of(m, lattice):
    x0, y0, dx, dy, nx, ny = lattice
    t = m.sample_grid((x0, y0), (dx, dy), (ny, nx), fields=("fraction",), tiles=True)["tile"].reshape(ny, nx)
    return t


def test_size_edges(spray3):
    m = spray3
    fine = SPRAY_LATTICE
    # tile 2 owns only the last lattice column: a window one node wide that ends at the lattice's edge cuts no cell
    last = fine[:4] + (49, 46)
    t = windows_of(m, last)
    assert (t[:, -1] == 2).all() and (t[:, :-1] != 2).all()
    ref, dev = check(m, last, what="last column")
    assert ref["count"] > 100 and not (dev["tile"] == 2).any() and (ref["quad"] == 2).any(1)[np.unique(ref["cell"])].sum() >= 4
    # tile 0 owns only the first lattice column: a window one node wide with an apron column
    first = (F(0.55), F(0.27), F(0.0119), F(0.0131), 20, 46)
    t = windows_of(m, first)
    assert (t[:, 0] == 0).all() and (t[:, 1:] != 0).all()
    ref, dev = check(m, first, what="first column")
    assert (dev["tile"] == 0).sum() >= 4 and (dev["tile"] == 1).sum() >= 4
    # a coarse lattice (dx = 15 h) whose nodes skip the middle strip altogether: its cells straddle that tile
    coarse = (F(0.25), F(0.27), F(0.3), F(0.0131), 4, 46)
    t = windows_of(m, coarse)
    assert sorted(np.unique(t).tolist()) == [0, 2], "the coarse lattice was meant to skip the middle strip"
    ref, dev = check(m, coarse, what="coarse")
    assert ref["count"] >= 4 and ((ref["quad"] == 0).any(1) & (ref["quad"] == 2).any(1))[np.unique(ref["cell"])].sum() >= 4
    # nx or ny of 1 and 2, and empty lattices
    for nx, ny in ((1, 46), (50, 1), (1, 1), (0, 46), (50, 0), (0, 0)):
        d = device(m, fine[:4] + (nx, ny), tiles=True)
        assert d["count"] == 0 and len(d["segments"]) == 0 and len(d["cell"]) == 0
    for nx, ny, x0, y0 in ((2, 46, F(0.55), F(0.27)), (50, 2, F(0.27), F(0.5)), (2, 2, F(0.551), F(0.5))):
        ref, dev = check(m, (x0, y0, fine[2], fine[3], nx, ny), what="%d x %d" % (nx, ny))
    assert check(m, (F(0.55), F(0.27), fine[2], fine[3], 2, 46), what="two columns on the cut")[0]["count"] >= 4
    # entirely outside the fluid, and entirely inside one tile
    ref, dev = check(m, (F(2.0), F(2.0), F(0.0119), F(0.0131), 30, 20), what="outside")
    assert ref["count"] == 0
    inside = (F(0.33), F(0.33), F(0.0119), F(0.0131), 17, 17)
    ref, dev = check(m, inside, what="inside one tile")
    assert ref["count"] > 20 and (ref["quad"] == 0).all()


def test_a_window_one_node_high():
    m = spray_multi("3 strips along y")
    one_row = (F(0.27), F(0.635), F(0.0119), F(0.0131), 50, 12)  # y = 0.635 is cell row 5031, the last of tile 1; row 1 (0.648) is tile 2's
    ref, dev = check(m, one_row, what="y strips")
    assert ref["count"] > 50 and (dev["tile"] == 1).sum() >= 4
    t = windows_of(m, one_row)
    assert (t[0] == 1).all() and (t[1:] == 2).all()
    m.close()


# ---- 5. capacity ------------------------------------------------------------------------------------------------------------------------------
def raw_call(m, lattice, iso, cap, seg, cell, tile, count, flags=0, kind=0, field=0):
    x0, y0, dx, dy, nx, ny = lattice
    o = _lib.SphxMultiContourOut()
    o.segments, o.cell, o.tile, o.count = (a.ctypes.data if a is not None else None for a in (seg, cell, tile, count))
    return m.L.sphx_multi_surface_contour(m.h, x0, y0, dx, dy, nx, ny, kind, field, iso, cap, flags, C.byref(o))


def test_capacity_and_count_only(spray_grid):
    m = spray_grid
    ref = reference(m, SPRAY_LATTICE)
    total = ref["count"]
    assert total > 300
    for cap in (0, 1, total - 1, total, total + 9):
        room = total + 16
        outs = []
        for _ in range(2):  # two calls return the same bytes
            seg, cell, tile, cnt = np.full((room, 4), -7.0, F), np.full(room, SENTINEL, np.uint32), np.full(room, -77, np.int32), np.zeros(1, np.uint32)
            assert raw_call(m, SPRAY_LATTICE, 0.5, cap, seg, cell, tile, cnt) == 0, m.L.sphx_multi_last_error(m.h)
            outs.append((seg.tobytes(), cell.tobytes(), tile.tobytes(), int(cnt[0])))
        assert outs[0] == outs[1]
        n = min(cap, total)
        assert cnt[0] == total
        assert np.array_equal(cell[:n], ref["cell"][:n]) and np.array_equal(tile[:n], ref["tile"][:n])
        assert np.array_equal(bits(seg[:n]), bits(ref["segments"][:n]).reshape(n, 4))
        assert (cell[n:] == SENTINEL).all() and (tile[n:] == -77).all() and (seg[n:] == -7.0).all(), "cap %d: written at or behind the capacity" % cap
    # the count alone: no array at all; segments alone; cells alone
    cnt = np.zeros(1, np.uint32)
    assert raw_call(m, SPRAY_LATTICE, 0.5, 0, None, None, None, cnt) == 0 and cnt[0] == total
    seg = np.full((total, 4), -7.0, F)
    assert raw_call(m, SPRAY_LATTICE, 0.5, total, seg, None, None, cnt) == 0 and np.array_equal(bits(seg), bits(ref["segments"]).reshape(total, 4))
    cell = np.full(total, SENTINEL, np.uint32)
    assert raw_call(m, SPRAY_LATTICE, 0.5, total, None, cell, None, cnt) == 0 and np.array_equal(cell, ref["cell"])
    # the wrapper: cap=None is two calls, the count and then the exact capacity
    d = device(m, SPRAY_LATTICE)
    assert d["count"] == total == len(d["segments"]) and "tile" not in d
    d = device(m, SPRAY_LATTICE, cap=10)
    assert d["count"] == total and len(d["cell"]) == 10 and np.array_equal(d["cell"], ref["cell"][:10])


# ---- 6. no side effects -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("band", ["a ring is left", "the band is spent"])
def test_contour_calls_leave_no_trace_in_the_run(band):
    """halo 10 with adaptive iteration counts: a ring is left at most calls.  A fixed halo of 7 cells with 2 density and 3 divergence
    iterations: from the second step on the divergence loop ends with valid = 0, and the call makes the exchange the next step_begin owes."""
    spent = band == "the band is spent"
    runs = []
    for calling in (False, True):
        if spent:
            m = new_multi(2, None, params=y.default_params(fixed_iterations=(2, 3)), halo=7, fixed_halo=True, invariant=True)
        else:
            m = new_multi(2)
        m.upload(POS)
        timer = y.TimeManager()
        stats, moved = [], 0
        for k in range(STEPS):
            stats.append(m.step(timer))
            if calling:
                if spent and k >= 1:
                    assert m.ghost_rings()["valid"] < 1, m.ghost_rings()  # the precondition of this case
                before = m.info()["exchanges"]
                d = device(m, DAM_LATTICE, field="fraction" if k % 2 else "density", iso=0.5 if k % 2 else 40.0)
                assert d["count"] > 40
                moved += m.info()["exchanges"] - before
                device(m, DAM_LATTICE, cap=0)
                assert m.info()["exchanges"] - before <= 1  # (the second call found a full band)
        if calling:
            assert moved >= STEPS - 1 if spent else moved < STEPS, moved
        d = m.download()
        order = np.argsort(d["ids"], kind="stable")
        digest = m.state_digest()
        m.step_begin(timer.simulation_step())
        runs.append(dict(stats=stats, d={k: v[order] for k, v in d.items()}, digest=digest, exchanges=m.info()["exchanges"], rebalances=m.info()["rebalances"]))
        m.close()
    a, b = runs
    for k in range(STEPS):
        assert a["stats"][k] == b["stats"][k], (k, a["stats"][k], b["stats"][k])
    for f in a["d"]:
        assert np.array_equal(bits(a["d"][f]), bits(b["d"][f])), f
    assert a["digest"] == b["digest"] and a["exchanges"] == b["exchanges"] and a["rebalances"] == b["rebalances"]


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------------------
def test_refusals_and_no_ops():
    bad, not_ready = _lib.ERR_INVALID_ARGUMENT, _lib.ERR_NOT_READY
    m = new_multi(2)
    L = m.L
    seg, cell, cnt = np.full((32, 4), -7.0, F), np.full(32, SENTINEL, np.uint32), np.full(1, 99, np.uint32)

    def call(x0=0.0, y0=0.0, dx=0.1, dy=0.1, nx=4, ny=4, kind=0, field=0, iso=0.5, cap=32, flags=0, out=True, count=True):
        o = _lib.SphxMultiContourOut(seg.ctypes.data, cell.ctypes.data, None, cnt.ctypes.data if count else None)
        rc = L.sphx_multi_surface_contour(m.h, x0, y0, dx, dy, nx, ny, kind, field, iso, cap, flags, C.byref(o) if out else None)
        return rc, L.sphx_multi_last_error(m.h).decode()

    # arguments first (they name the argument), before the first upload too
    for kw, word in ((dict(out=False), "out is NULL"), (dict(count=False), "count"), (dict(kind=3), "kernel_kind"), (dict(field=2), "field"), (dict(field=-1), "field"),
                     (dict(flags=1), "flags"), (dict(flags=2), "flags"), (dict(iso=float("nan")), "iso"), (dict(iso=float("inf")), "iso"),
                     (dict(x0=float("nan")), "x0 / y0"), (dict(y0=float("inf")), "x0 / y0"), (dict(dx=0.0), "dx"), (dict(dx=float("inf")), "dx"),
                     (dict(dy=-1.0), "dy"), (dict(dy=float("nan")), "dy"), (dict(nx=1 << 16, ny=1 << 15), "nx * ny")):
        rc, msg = call(**kw)
        assert rc == bad and word in msg, (kw, msg)
    assert cnt[0] == 99 and (cell == SENTINEL).all()
    # successful calls with count 0 once the arguments pass, whatever the state
    for kw in (dict(nx=0), dict(ny=0), dict(nx=1), dict(ny=1), dict(nx=0, ny=0)):
        cnt[0] = 99
        assert call(**kw)[0] == 0 and cnt[0] == 0
    # before the first upload
    rc, msg = call()
    assert rc == not_ready and "upload" in msg
    m.upload(POS)
    assert call()[0] == 0
    # between step_begin and step_finish
    timer = y.TimeManager()
    m.step_begin(timer.simulation_step())
    before = m.info()["exchanges"]
    rc, msg = call()
    assert rc == not_ready and "step" in msg and m.info()["exchanges"] == before
    m.step_finish(F(0.001))
    assert call()[0] == 0
    # the wrapper names a bad field itself
    with pytest.raises(ValueError):
        m.contour((0.0, 0.0), 0.1, (4, 4), field="pressure")
    # the seam: a plain context is refused, the calls come in their order
    ctx = y.SphxContext()
    win = (C.c_uint32 * 4)()
    assert L.sphx_tile_contour_sample(ctx.h, 0.0, 0.0, 0.1, 0.1, 4, 4, 0, 0, win) == bad and "not a tile context" in L.sphx_last_error(ctx.h).decode()
    assert L.sphx_tile_contour_cut(ctx.h, 0.5, 4, None, 0) == bad and L.sphx_tile_contour_border_fetch(ctx.h, None, 0) == bad
    ctx.close()
    t = m.tile_context(0)
    n = C.c_uint32()
    assert L.sphx_tile_contour_cut(t.h, 0.5, 4, None, 0) == not_ready and L.sphx_tile_contour_fetch(t.h, None, None, C.byref(n)) == not_ready
    assert L.sphx_tile_contour_sample(t.h, 0.0, 0.0, 0.1, 0.1, 4, 4, 7, 0, win) == bad and L.sphx_tile_contour_sample(t.h, 0.0, 0.0, 0.1, 0.1, 4, 4, 0, 5, win) == bad
    m.close()


def test_solver_object_reaches_the_tiled_contour():
    w = y.FluidParticleWorld()
    w.reset_fluid(1.0)
    s = y.DFSPHMultiSolver(w, [0, 0])
    t = y.TimeManager()
    s.simulation_steps(w, t, 5, sync_world=False)
    m = s.multi()
    ref = reference(m, DAM_LATTICE)
    x0, y0, dx, dy, nx, ny = DAM_LATTICE
    assert_same(s.contour((x0, y0), (dx, dy), (ny, nx), tiles=True), ref, "the solver object's tiles")
    s.close()


# ---- 8. one process per tile ----------------------------------------------------------------------------------------------------------------
def test_rank_mode_parts_merge_to_the_in_process_run(tmp_path):
    """Two processes over gloo (the halo records) and the shared segment (the scalars, the windows' borders), both on device 0.  Each rank
    returns its own part; the parts, folded with contour_merge, are the bytes of the in-process devices=[0, 0] run.  A deliberately small
    cap on one rank makes the merge return SPHX_ERR_CAPACITY with the right total."""
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1", "--master-port", "29571",
           os.path.join(HERE, "contour_multi_rank_worker.py"), str(tmp_path), str(STEPS)]
    p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    r = [np.load(tmp_path / f"rank{k}.npz") for k in range(2)]
    lat = r[0]["lattice"].tolist()
    lattice = tuple(F(v) for v in lat[:4]) + (int(lat[4]), int(lat[5]))
    m = new_multi(2)
    m.upload(POS)
    m.steps(y.TimeManager(), STEPS)
    want = device(m, lattice, tiles=True)
    m.close()
    assert want["count"] > 40
    for k in range(2):  # the raw call without out->cell was refused on both ranks before any exchange (the worker checked that too)
        assert int(r[k]["refused_without_cell"]) == _lib.ERR_INVALID_ARGUMENT
    parts = [dict(segments=r[k]["segments"].view(F), cell=r[k]["cell"], tile=r[k]["tile"], count=int(r[k]["count"])) for k in range(2)]
    for k, part in enumerate(parts):
        assert part["count"] == len(part["cell"]) == (want["tile"] == k).sum() > 0 and (part["tile"] == k).all()
        assert (np.diff(part["cell"].astype(np.int64)) >= 0).all()
    got = y.contour_merge(parts)
    assert got["count"] == want["count"]
    for f in ("segments", "cell", "tile"):
        assert np.array_equal(bits(got[f]), bits(want[f])), f
    # rank 1 was also asked with a capacity three short of its count
    short = dict(segments=r[1]["short_segments"].view(F), cell=r[1]["short_cell"], tile=r[1]["short_tile"], count=int(r[1]["short_count"]))
    assert short["count"] == parts[1]["count"] and len(short["cell"]) == short["count"] - 3 and np.array_equal(short["cell"], parts[1]["cell"][:-3])
    with pytest.raises(y.SphxError) as e:
        y.contour_merge([parts[0], short])
    assert e.value.code == _lib.ERR_CAPACITY and e.value.count == want["count"]
