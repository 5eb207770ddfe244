"""sphx_append / sphx_remove on the device (include/sphx.h, "emitting and draining fluid").  The rule everything is tested against: apart
from the particle ids, an edit leaves the state that download, filter / concatenate on the host (tests/edit_reference.py) and a fresh
sphx_upload leave in a context with the same history, and every later step is bit-identical to that context's — and to the oracle's,
edited with set_particles.  The removal counts, the oracle's finiteness and its neighbour flags on these scenes are checked without a
GPU in tests/test_edit_host.py."""
import json
import os
import subprocess

import numpy as np
import pytest
from util import assert_bits_equal, assert_same_neighbors

import edit_reference as ref
import yasph2d_amd as y
from oracle.oracle import Oracle
from yasph2d_amd import _lib

pytestmark = pytest.mark.gpu

F = np.float32
INF = float("inf")
NAN = float("nan")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "dam_break_4050.npz"))
POS, BOUNDARY = GOLD["in_pos"], GOLD["in_boundary"]
DIAM = F(0.01)
HARNESS = os.path.join(os.path.dirname(os.path.abspath(y.__file__)), "sphx_harness")


def same_bits(a, b, what):
    """exact equality of two arrays that may hold NaN and signed zeros: compared as raw words"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), what


def block(nx, ny, x, y0, spacing=F(0.0111)):
    g = np.stack(np.meshgrid(np.arange(nx), np.arange(ny)), -1).reshape(-1, 2).astype(F)
    return (np.array([x, y0], F) + g * F(spacing)).astype(F)


# ---- 1. the compaction alone (no stepping: upload order = device order) ---------------------------------------------------------------
def patterns(n):
    """name -> mask of the particles to remove"""
    i = np.arange(n)
    rng = np.random.default_rng(1234 + n)
    return {
        "none": np.zeros(n, bool), "all": np.ones(n, bool), "odd": i % 2 == 1, "even": i % 2 == 0, "first only": i == 0, "last only": i == n - 1,
        "all but last": i != n - 1, "first wave": i < 64, "last (partial) wave": i >= ((n - 1) // 64) * 64, "every 64th": i % 64 == 0,
        "random 0.5": rng.random(n) < 0.5, "random 0.01": rng.random(n) < 0.01,
    }


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 12289])
def test_compaction_is_the_numpy_filter_in_order(n):
    """a wavefront, a workgroup, 16 workgroups and 48 + 1, each with one particle less and one more; the pattern is in x, the index in y
    and in the velocity"""
    ctx = y.SphxContext()
    i = np.arange(n)
    vel = np.stack([i, -i], -1).astype(F)
    ids = i.astype(np.uint32)
    for name, gone in patterns(n).items():
        pos = np.stack([np.where(gone, F(0.75), F(0.25)), i * F(2.0 ** -14)], -1).astype(F)
        for outside, rect in ((False, (0.5, -INF, 1.0, INF)), (True, (0.0, -INF, 0.5, INF))):
            what = "n = %d, %s%s" % (n, name, ", OUTSIDE" if outside else "")
            ctx.upload(pos, vel)
            rp, rv, ri, removed = ref.remove(pos, vel, ids, rect, outside)
            assert removed == int(gone.sum()), what
            assert ctx.remove(rect, outside=outside) == removed, what
            assert ctx.n == n - removed, what
            d = ctx.download()
            same_bits(d["pos"], rp, what + ": positions")
            same_bits(d["vel"], rv, what + ": velocities")
            np.testing.assert_array_equal(d["ids"], ri, what + ": ids")


# ---- 2. the predicate's edges ---------------------------------------------------------------------------------------------------------
def edge_points():
    lo, hi, den = F(0.25), F(0.75), F(1e-45)
    below = lambda v: np.nextafter(F(v), F(-INF))  # noqa: E731
    pts = [(lo, 0.5), (hi, 0.5), (0.5, lo), (0.5, hi), (below(lo), 0.5), (below(hi), 0.5), (0.5, below(lo)), (0.5, below(hi)), (lo, lo), (hi, hi),
           (0.0, 0.0), (-0.0, -0.0), (0.0, -0.0), (den, den), (-den, den), (den, -den), (NAN, 0.5), (0.5, NAN), (NAN, NAN), (INF, 0.5), (-INF, 0.5),
           (0.5, INF), (0.5, -INF), (INF, INF), (0.5, 0.5), (1.0, 1.0), (-1.0, 2.0)]
    return np.array(pts, F)


EDGE_RECTS = [
    [(0.25, 0.25, 0.75, 0.75)],
    [(0.0, 0.0, 1.0, 1.0)],
    [(-0.0, -0.0, 1e-45, 1e-45)],
    [(-INF, -INF, INF, INF)],
    [(0.0, -INF, INF, INF)],
    [(-INF, -INF, 0.0, INF)],
    [(-INF, 0.5, INF, INF)],
    [(0.75, 0.25, 0.25, 0.75)],  # x0 > x1: empty
    [],
    # eight overlapping rectangles: a particle in two of them is removed once
    [(0.0, 0.0, 0.5, 0.5), (0.25, 0.25, 0.75, 0.75), (0.5, 0.5, 1.0, 1.0), (0.5, -INF, 0.6, INF), (-INF, 0.9, INF, 1.1), (0.25, 0.5, 0.3, 0.6),
     (-1.5, 1.5, -0.5, 2.5), (INF, INF, INF, INF)],
]


@pytest.mark.parametrize("outside", [False, True])
def test_predicate_edges_against_numpy(outside):
    pts = edge_points()
    vel = np.stack([np.arange(len(pts)), np.arange(len(pts)) + 100], -1).astype(F)
    ids = np.arange(len(pts), dtype=np.uint32)
    ctx = y.SphxContext()
    seen = set()
    for rects in EDGE_RECTS:
        ctx.upload(pts, vel)
        rp, rv, ri, removed = ref.remove(pts, vel, ids, rects, outside)
        assert ctx.remove(rects, outside=outside) == removed, rects
        d = ctx.download()
        assert ctx.n == len(pts) - removed
        same_bits(d["pos"], rp, rects)
        same_bits(d["vel"], rv, rects)
        np.testing.assert_array_equal(d["ids"], ri)
        seen.add(removed)
    assert len(seen) >= 5  # the cases tell the rectangles apart
    # refused: nine rectangles, a NaN bound, unknown flag bits; the set stays as it is
    ctx.upload(pts, vel)
    for bad in ([(0.0, 0.0, 1.0, 1.0)] * 9, (0.0, NAN, 1.0, 1.0), [(0.0, 0.0, 1.0, 1.0), (0.0, 0.0, NAN, 1.0)]):
        with pytest.raises(y.SphxError) as e:
            ctx.remove(bad, outside=outside)
        assert e.value.code == _lib.ERR_INVALID_ARGUMENT
    r = _lib.SphxRect(0.0, 0.0, 1.0, 1.0)
    assert ctx.L.sphx_remove(ctx.h, r, 1, 2, None) == _lib.ERR_INVALID_ARGUMENT
    assert ctx.L.sphx_remove(ctx.h, None, 1, 0, None) == _lib.ERR_INVALID_ARGUMENT
    assert ctx.n == len(pts)
    # out_removed may be NULL
    assert ctx.L.sphx_remove(ctx.h, r, 1, 0, None) == _lib.OK and ctx.n == len(pts) - int(ref.removed_mask(pts, (0.0, 0.0, 1.0, 1.0)).sum())


# ---- 3. equivalence after real steps: X edits on the device, Y makes the round trip, the oracle is edited with set_particles --------
STAT_KEYS = ("density_iterations", "divergence_iterations", "warmstart_density", "warmstart_divergence")


def dfsph_step(ctx, timer):
    vmax = ctx.step_begin(timer.simulation_step(), timer.law(DIAM))
    return ctx.step_finish(y.duration_as_secs_f32(timer.update_simulation_step(DIAM, vmax)))


class Trio:
    def __init__(self, reserve=0):
        self.X, self.Y, self.O = y.SphxContext(), y.SphxContext(), Oracle()
        for c in (self.X, self.Y):
            if reserve:
                c._chk(c.L.sphx_reserve(c.h, reserve))
            c.set_boundary(BOUNDARY)
            c.upload(POS)
        self.O.set_boundary(BOUNDARY)
        self.O.set_particles(POS)
        self.tx, self.ty = y.TimeManager(), y.TimeManager()
        self.x_of_y = np.arange(len(POS), dtype=np.uint32)  # the id X holds for the particle Y numbers k
        self.issued = len(POS)

    def step(self, what=""):
        sx, sy, so = dfsph_step(self.X, self.tx), dfsph_step(self.Y, self.ty), self.O.dfsph_step()
        assert self.tx.simulation_step_ns() == self.ty.simulation_step_ns() == self.O.timer_step_ns(), what
        for k in STAT_KEYS:
            assert sx[k] == sy[k] == so[k], (what, k, sx[k], sy[k], so[k])
        assert so["neighbor_flags"] == 0, what
        return sx

    def edit(self, rects=None, outside=False, new_pos=None, new_vel=None):
        """append new_pos (if any), then remove by rects (if any): X with the new calls, Y and the oracle through the host.
        -> (appended, removed)"""
        n0 = self.X.n
        first = None
        if new_pos is not None:
            first = self.X.append(new_pos, new_vel)
            assert first == self.issued
            self.issued += len(new_pos)
        removed = self.X.remove(rects, outside=outside) if rects is not None else 0
        if new_pos is None and removed == 0:
            return 0, 0  # nothing changed: no round trip either
        d = self.Y.download()
        po, vo = self.O.positions(), self.O.velocities()
        ids = self.x_of_y[d["ids"]]
        p, v = d["pos"], d["vel"]
        if new_pos is not None:
            p, v, ids = ref.append(p, v, ids, new_pos, new_vel, first)
            po, vo = np.concatenate([po, p[len(po):]]), np.concatenate([vo, v[len(vo):]])
        if rects is not None:
            gone = ref.removed_mask(po, rects, outside)
            p, v, ids, r = ref.remove(p, v, ids, rects, outside)
            assert r == removed == int(gone.sum())
            po, vo = po[~gone], vo[~gone]
        self.Y.upload(p, v)
        self.O.set_particles(po, vo)
        self.x_of_y = ids
        assert self.X.n == self.Y.n == self.O.n == n0 + (len(new_pos) if new_pos is not None else 0) - removed
        return (len(new_pos) if new_pos is not None else 0), removed

    def compare(self, what):
        dx, dy = self.X.download(), self.Y.download()
        for name, ref_arr in (("pos", self.O.positions()), ("vel", self.O.velocities()), ("density", self.O.densities())):
            assert_bits_equal(dx[name], dy[name], "%s: %s, device edit against round trip" % (what, name))
            assert_bits_equal(dx[name], ref_arr, "%s: %s against the oracle" % (what, name))
        sx, sy = self.X.download_solver_state(), self.Y.download_solver_state()
        for name, ref_arr in (("kappa", self.O.kappa()), ("stiffness", self.O.stiffness())):
            assert_bits_equal(sx[name], sy[name], "%s: %s, device edit against round trip" % (what, name))
            assert_bits_equal(sx[name], ref_arr, "%s: %s against the oracle" % (what, name))
        assert_bits_equal(sx["alpha"], sy["alpha"], what + ": alpha")
        nx = self.X.download_neighbors()
        assert_same_neighbors(nx, self.Y.download_neighbors())
        assert_same_neighbors(nx, self.O.neighbors())
        np.testing.assert_array_equal(dy["ids"], self.O.ids(), what + ": the round trip's ids")
        np.testing.assert_array_equal(dx["ids"], self.x_of_y[dy["ids"]], what + ": ids kept by the device edit")
        assert len(np.unique(dx["ids"])) == len(dx["ids"])


@pytest.mark.parametrize("rects,outside,removed", [
    ([(0.6, -INF, INF, INF)], False, 200),
    ([(0.2, 0.4, 0.7, 0.9)], False, 1415),
    ([(-INF, -INF, INF, 0.7)], False, 845),
    ([(0, 1, 0.3, INF), (0.6, -INF, INF, 0.8)], False, 874),
    ([(0, 0.5, 0.7, 1.3)], True, 505),
])
def test_remove_after_150_steps_equals_the_round_trip(rects, outside, removed):
    t = Trio()
    for s in range(150):
        t.step("step %d" % s)
    assert np.abs(t.X.download_solver_state()["stiffness"]).max() > 0  # (the slot-bound values are not trivial)
    assert t.edit(rects, outside) == (0, removed)
    st = t.step("first step after the edit")
    assert st["flags"] & y.FLAG_WARMUP
    for s in range(39):
        st = t.step("step %d after the edit" % (s + 1))
        assert not st["flags"] & y.FLAG_WARMUP
    t.compare("40 steps after removing %d" % removed)


@pytest.mark.parametrize("rects,outside,removed", [([(1.0, -INF, INF, INF)], False, 1665), ([(0, 0, 1.5, 2.5)], True, 1037)])
def test_remove_after_600_steps_with_the_divergence_warm_start_firing(rects, outside, removed):
    t = Trio()
    for s in range(600):
        t.step("step %d" % s)
    assert t.edit(rects, outside) == (0, removed)
    twice = sum(t.step("step %d after the edit" % s)["divergence_iterations"] == 2 for s in range(60))
    assert twice == 60
    t.compare("60 steps after removing %d" % removed)


@pytest.mark.parametrize("reserve", [0, 2 * len(POS)], ids=["reallocation", "in place"])
def test_append_after_150_steps_equals_the_round_trip(reserve):
    """the 20 x 20 block of test_adding_particles_mid_run... (tests/test_gpu_edges.py), once into exact capacity and once into reserved room"""
    t = Trio(reserve)
    for s in range(150):
        t.step("step %d" % s)
    extra = block(20, 20, 1.2, 1.0)
    assert t.edit(new_pos=extra) == (400, 0)
    assert t.X.n == len(POS) + 400
    np.testing.assert_array_equal(t.X.download()["ids"][-400:], len(POS) + np.arange(400))  # before any step: behind the present particles
    same_bits(t.X.download()["pos"][-400:], extra, "appended positions")
    assert t.step("first step after the edit")["flags"] & y.FLAG_WARMUP
    for s in range(39):
        t.step("step %d after the edit" % (s + 1))
    t.compare("40 steps after appending 400")


def test_emitter_and_drain_over_60_steps():
    t = Trio()
    for s in range(150):
        t.step("step %d" % s)
    down = np.tile(np.array([[0.0, -1.0]], F), (64, 1))
    emitted = drained = 0
    for s in range(60):
        n0 = t.X.n
        new = block(8, 8, F(1.0) + F(0.1) * F(s // 5), 1.0) if s % 5 == 0 and s < 40 else None
        a, r = t.edit([(-INF, -INF, INF, 0.62)], False, new, down if new is not None else None)
        emitted, drained = emitted + a, drained + r
        assert (a, r) == (0, 0) or t.X.n != n0  # (no edit brings the count back: the remove-k-append-k corner has a test of its own)
        st = t.step("emitter step %d" % s)
        assert bool(st["flags"] & y.FLAG_WARMUP) == ((a, r) != (0, 0))
    assert (emitted, drained, t.X.n) == (8 * 64, 648, 3914)
    t.compare("emitter and drain")
    assert t.X.download()["ids"].max() == len(POS) + 8 * 64 - 1


def test_wcsph_remove_equals_the_round_trip():
    """X against Y only.  600 WCSPH steps bring 195 particles past x = 0.6 (the oracle's figure, tests/test_edit_host.py)."""
    X, Y = y.SphxContext(), y.SphxContext()
    timers = y.TimeManager(cfl_factor=0.2), y.TimeManager(cfl_factor=0.2)
    for c in (X, Y):
        c.set_boundary(BOUNDARY)
        c.upload(POS)

    def step():
        out = []
        for c, t in zip((X, Y), timers):
            vmax = c.wcsph_step_begin(t.simulation_step())
            out.append(c.wcsph_step_finish(y.duration_as_secs_f32(t.update_simulation_step(DIAM, vmax))))
        assert timers[0].simulation_step_ns() == timers[1].simulation_step_ns()
        assert out[0]["neighbor_entries"] == out[1]["neighbor_entries"]

    for _ in range(600):
        step()
    d = Y.download()
    p, v, ids, removed = ref.remove(d["pos"], d["vel"], d["ids"], (0.6, -INF, INF, INF))
    assert removed == 195 and X.remove((0.6, -INF, INF, INF)) == 195
    Y.upload(p, v)
    for _ in range(30):
        step()
    dx, dy = X.download(), Y.download()
    for name in ("pos", "vel", "density"):
        assert_bits_equal(dx[name], dy[name], "WCSPH " + name)
    np.testing.assert_array_equal(dx["ids"], ids[dy["ids"]])
    assert_same_neighbors(X.download_neighbors(), Y.download_neighbors())


# ---- 4. the corner: the count comes back to the cached length ---------------------------------------------------------------------------
def test_remove_k_append_k_runs_the_warm_up_block():
    """The one deliberate difference from a round trip (which would find the count unchanged and walk the lists of another set).  The
    oracle is driven through the same block by hand: set_particles zeroes its densities and leaves the lists alone, so the three
    calls of dfsph.rs:423-427 follow it."""
    X, O = y.SphxContext(), Oracle()
    X.set_boundary(BOUNDARY)
    X.upload(POS)
    O.set_boundary(BOUNDARY)
    O.set_particles(POS)
    timer = y.TimeManager()
    for _ in range(150):
        dfsph_step(X, timer)
        O.dfsph_step()
    extra = block(20, 10, 1.2, 1.0)
    assert X.remove((0.6, -INF, INF, INF)) == 200
    assert X.append(extra) == len(POS)
    assert X.n == len(POS)
    po, vo = O.positions(), O.velocities()
    gone = ref.removed_mask(po, (0.6, -INF, INF, INF))
    O.set_particles(np.concatenate([po[~gone], extra]), np.concatenate([vo[~gone], np.zeros_like(extra)]))
    O.update_neighborhood()
    O.update_densities()
    O.compute_alpha()
    for s in range(20):
        st, so = dfsph_step(X, timer), O.dfsph_step()
        assert bool(st["flags"] & y.FLAG_WARMUP) == (s == 0)
        assert timer.simulation_step_ns() == O.timer_step_ns()
        for k in STAT_KEYS:
            assert st[k] == so[k], (s, k, st[k], so[k])
    d, ss = X.download(), X.download_solver_state()
    assert_bits_equal(d["pos"], O.positions(), "corner: positions")
    assert_bits_equal(d["vel"], O.velocities(), "corner: velocities")
    assert_bits_equal(d["density"], O.densities(), "corner: densities")
    assert_bits_equal(ss["kappa"], O.kappa(), "corner: kappa")
    assert_bits_equal(ss["stiffness"], O.stiffness(), "corner: stiffness")
    assert_same_neighbors(X.download_neighbors(), O.neighbors())


# ---- 5. nothing removed, nothing appended ---------------------------------------------------------------------------------------------
def test_an_edit_that_changes_nothing_leaves_the_context_untouched():
    A, B = y.SphxContext(), y.SphxContext()
    ta, tb = y.TimeManager(), y.TimeManager()
    for c in (A, B):
        c.set_boundary(BOUNDARY)
        c.upload(POS)
    for _ in range(20):
        dfsph_step(A, ta)
        dfsph_step(B, tb)
    assert A.remove((5.0, 5.0, 6.0, 6.0)) == 0
    assert A.remove([]) == 0
    assert A.remove((-INF, -INF, INF, INF), outside=True) == 0
    assert A.append(np.zeros((0, 2), F)) == len(POS)
    assert A.n == len(POS)
    pts = POS[::97] + F(0.003)
    sa, sb = A.sample(pts), B.sample(pts)  # still answers: the lists and the densities belong to the positions
    for k in sa:
        same_bits(sa[k], sb[k], "sample " + k)
    for s in range(3):
        st_a, st_b = dfsph_step(A, ta), dfsph_step(B, tb)
        assert st_a == st_b and not st_a["flags"] & y.FLAG_WARMUP
    da, db = A.download(), B.download()
    for k in da:
        same_bits(da[k], db[k], "twin " + k)
    assert_same_neighbors(A.download_neighbors(), B.download_neighbors())


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------------
def refused(code, fn, *args, **kw):
    with pytest.raises(y.SphxError) as e:
        fn(*args, **kw)
    assert e.value.code == code, e.value
    return str(e.value)


def test_refusals():
    rect, pts = (0.6, -INF, INF, INF), block(2, 2, 1.2, 1.0)
    ctx = y.SphxContext()
    # before the first upload; an upload of zero particles counts as one
    assert "no particles uploaded" in refused(_lib.ERR_NOT_READY, ctx.remove, rect)
    assert "no particles uploaded" in refused(_lib.ERR_NOT_READY, ctx.append, pts)
    ctx.upload(np.zeros((0, 2), F))
    assert ctx.remove(rect) == 0 and ctx.remove(rect, outside=True) == 0
    assert ctx.append(pts) == 0 and ctx.n == 4
    np.testing.assert_array_equal(ctx.download()["ids"], np.arange(4))
    assert ctx.remove((-INF, -INF, INF, INF)) == 4 and ctx.n == 0  # N = 0 is legal
    assert ctx.append(pts[:1]) == 4  # ids are never reused
    # inside a step, either solver
    ctx.set_boundary(BOUNDARY)
    ctx.upload(POS)
    timer = y.TimeManager()
    vmax = ctx.step_begin(timer.simulation_step(), timer.law(DIAM))
    assert "between step_begin and step_finish" in refused(_lib.ERR_NOT_READY, ctx.remove, rect)
    assert "between step_begin and step_finish" in refused(_lib.ERR_NOT_READY, ctx.append, pts)
    ctx.step_finish(y.duration_as_secs_f32(timer.update_simulation_step(DIAM, vmax)))
    w = y.SphxContext()
    w.set_boundary(BOUNDARY)
    w.upload(POS)
    tw = y.TimeManager(cfl_factor=0.2)
    vmax = w.wcsph_step_begin(tw.simulation_step())
    refused(_lib.ERR_NOT_READY, w.remove, rect)
    refused(_lib.ERR_NOT_READY, w.append, pts)
    w.wcsph_step_finish(y.duration_as_secs_f32(tw.update_simulation_step(DIAM, vmax)))
    assert w.remove((0.3, -INF, INF, INF)) > 0
    # sampling waits for a build of the new set; render and download work at once
    assert ctx.remove(rect) == 0 and ctx.sample(POS[:4])["count"].shape == (4,)
    gone = ctx.remove((0.3, -INF, INF, INF))
    assert gone > 0
    assert "sphx_remove" in refused(_lib.ERR_NOT_READY, ctx.sample, POS[:4])
    owner = ctx.render(width=320, height=180, owner=True, rgba=False)
    fluid = owner[owner < _lib.RENDER_BOUNDARY]
    assert fluid.size and fluid.max() < ctx.n == len(POS) - gone
    ctx.append(pts)
    assert "sphx_append" in refused(_lib.ERR_NOT_READY, ctx.sample, POS[:4])
    # a tile context, with the wording sphx_render uses; tiling-invariant mode
    tc = y.SphxContext()
    assert tc.L.sphx_tile_configure(tc.h, 0, 0, 65536, 4, 0, 0) == _lib.OK
    assert "not available on a tile context (its arrays hold ghosts and miss the particles other tiles own)" in refused(
        _lib.ERR_INVALID_ARGUMENT, tc.remove, rect)
    assert "not available on a tile context" in refused(_lib.ERR_INVALID_ARGUMENT, tc.append, pts)
    ti = y.SphxContext()
    ti.upload(POS)
    ti.set_tiling_invariant(True)
    assert "tiling-invariant" in refused(_lib.ERR_INVALID_ARGUMENT, ti.remove, rect)
    assert "tiling-invariant" in refused(_lib.ERR_INVALID_ARGUMENT, ti.append, pts)
    ti.set_tiling_invariant(False)
    assert ti.remove(rect) == 0


# ---- 7. the host mirror and the harness ---------------------------------------------------------------------------------------------
def test_solver_object_edits_without_a_re_upload():
    w = y.FluidParticleWorld()
    w.reset_fluid(1.0)
    n = w.num_dynamic_particles
    solver, timer = y.DFSPHSolver(w), y.TimeManager()
    rect = (-INF, -INF, INF, 0.65)
    assert "first step" in refused(_lib.ERR_NOT_READY, solver.remove, w, rect)
    solver.simulation_steps(w, timer, 150, sync_world=False)
    solver.sync_world(w)
    ids0, pos0 = w.particle_ids, w.positions
    low = ids0[ref.removed_mask(pos0, rect)]
    assert 0 < len(low) < n
    assert solver.remove(w, rect, sync_world=False) == len(low)
    assert w.num_dynamic_particles == n - len(low)
    extra = block(8, 8, 1.2, 1.0)
    assert solver.append(w, extra, np.tile(np.array([[0.0, -1.0]], F), (64, 1)), sync_world=False) == n
    assert w.num_dynamic_particles == n - len(low) + 64 == solver.context().n
    solver.simulation_steps(w, timer, 10, sync_world=False)  # (a re-upload would number the particles afresh: 0 .. count - 1)
    solver.sync_world(w)
    ids = np.sort(w.particle_ids)
    np.testing.assert_array_equal(ids, np.concatenate([np.setdiff1d(ids0, low), n + np.arange(64)]).astype(np.uint32))
    assert np.isfinite(w.positions).all() and len(w.positions) == n - len(low) + 64
    # with sync_world the arrays are current at once
    gone = solver.remove(w, (1.2, 0.9, 1.3, 1.2), sync_world=True)
    assert len(w.positions) == solver.context().n == n - len(low) + 64 - gone
    assert not ref.removed_mask(w.positions, (1.2, 0.9, 1.3, 1.2)).any()
    np.testing.assert_array_equal(w.particle_ids, solver.context().download()["ids"])
    # an edit of the host world is waiting for its upload
    w.add_fluid_rect(1.5, 1.0, 0.05, 0.05, 0.0)
    assert "edited" in refused(_lib.ERR_NOT_READY, solver.append, w, extra)
    solver.simulation_step(w, timer)
    assert solver.remove(w, (5.0, 5.0, 6.0, 6.0)) == 0


def test_harness_emit_and_drain_add_up():
    out = subprocess.run([HARNESS, "--particles", "4050", "--steps", "60", "--warmup", "0", "--emit", "1.0,1.0,0.08,0.08:every=5:until=40:vel=0,-1",
                          "--drain", "-inf,-inf,inf,0.62"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    res = json.loads(out.stdout.strip().splitlines()[-1])
    assert res["emitted"] > 0 and res["emitted"] % 7 == 0  # (edits start before step 1: 5, 10, ... 35)
    assert res["drained"] >= 0
    assert res["final_particles"] == res["particles"] + res["emitted"] - res["drained"]
    assert res["particles"] == 4050
