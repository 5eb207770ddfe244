"""Neighbour queries on the device (sphx_query_radius / sphx_select): every output bit for bit against the numpy restatement of the
contract (tests/query_reference.py) applied to the device's own download() and download_boundary() — lists, sizes across every seam, a
dense cell, the capacity rule, device pointers, the state rules and argument errors of include/sphx.h, no side effects on a run, the tie
to sphx_remove and sphx_track_*, and the harness's CSVs.  No tolerance anywhere."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import query_reference as qr
import sample_reference as sr
import yasph2d_amd as y
from util import dam_break
from yasph2d_amd import _lib

pytestmark = pytest.mark.gpu

F = np.float32
DIAM = F(0.01)
HARNESS = os.path.join(os.path.dirname(os.path.abspath(y.__file__)), "sphx_harness")
OK, E_ARG, E_READY = _lib.OK, _lib.ERR_INVALID_ARGUMENT, _lib.ERR_NOT_READY
LISTS = ("offsets", "index", "id", "dist_sq", "nearest", "nearest_dist_sq", "count")
SENTINEL = 0xA5A5A5A5


def dfsph_steps(ctx, timer, k):
    for _ in range(k):
        vmax = ctx.step_begin(timer.simulation_step(), timer.law(DIAM))
        ctx.step_finish(y.duration_as_secs_f32(timer.update_simulation_step(DIAM, vmax)))


def wcsph_steps(ctx, timer, k):
    for _ in range(k):
        vmax = ctx.wcsph_step_begin(timer.simulation_step())
        ctx.wcsph_step_finish(y.duration_as_secs_f32(timer.update_simulation_step(DIAM, vmax)))


def scene_ctx(**kw):
    pos, bnd = dam_break()
    ctx = y.SphxContext(**kw)
    ctx.set_boundary(bnd)
    ctx.upload(pos)
    return ctx


def state_of(ctx):
    d = ctx.download()
    assert not ctx.last_flags() & y.FLAG_STRAY_PARTICLES
    bnd, bid = ctx.download_boundary()
    return dict(pos=d["pos"], ids=d["ids"], boundary=bnd, boundary_ids=bid)


def point_sets(st, seed, h):
    """random points over the fluid's bounds plus a margin, points exactly on particles (of both sets), one point 64 times, and a NaN, an
    infinite and a far point -> (points, slices of the four groups)"""
    rng = np.random.default_rng(seed)
    pos, bnd = st["pos"], st["boundary"]
    lo, hi = pos.min(0) - 3 * h, pos.max(0) + 3 * h
    groups = [(lo + rng.random((1500, 2)) * (hi - lo)).astype(F),
              np.concatenate([pos[rng.choice(len(pos), 300, replace=False)], bnd[rng.choice(len(bnd), 200, replace=False)]]),
              np.repeat(pos[len(pos) // 2][None, :] + F(0.25) * h, 64, 0).astype(F),
              np.array([[np.nan, 0.5], [0.5, np.nan], [np.inf, 0.5], [-np.inf, np.inf], [1e6, 1e6], [-150.0, -150.0], [3.4e38, -3.4e38]], F)]
    ends = np.cumsum([len(g) for g in groups])
    return np.concatenate(groups).astype(F), [slice(a, b) for a, b in zip(np.concatenate(([0], ends[:-1])), ends)]


def assert_same(dev, ref, what, keys=LISTS):
    for k in keys:
        a, b = np.asarray(dev[k]), np.asarray(ref[k])
        if a.dtype == F:
            a, b = a.view(np.uint32), b.astype(F).view(np.uint32)
        if a.dtype.kind == "i" and a.ndim:  # (torch has no unsigned types: the same words)
            a = a.view(np.dtype("u%d" % a.itemsize))
        assert a.shape == b.shape and np.array_equal(a.astype(np.uint64), b.astype(np.uint64)), "%s: %s differs" % (what, k)


class Scene:
    def __init__(self, ctx):
        self.ctx = ctx
        self.K = sr.Constants(ctx.params, ctx.constants())
        self.h = self.K.h
        self.st = state_of(ctx)
        self.pts, self.groups = point_sets(self.st, 11, self.h)
        self._ref = {}

    def ref(self, radius, boundary):
        key = (float(radius), boundary)
        if key not in self._ref:
            self._ref[key] = qr.query32(self.K, self.st, self.pts, radius, boundary)
        return self._ref[key]


@pytest.fixture(scope="module")
def dfsph():
    ctx = scene_ctx()
    dfsph_steps(ctx, y.TimeManager(), 60)
    return Scene(ctx)


@pytest.fixture(scope="module")
def wcsph():
    ctx = scene_ctx()
    wcsph_steps(ctx, y.TimeManager(cfl_factor=0.2), 60)
    return Scene(ctx)


@pytest.fixture(scope="module")
def built():
    ctx = scene_ctx()
    ctx.update_neighborhood()
    ctx.update_densities(y.KERNEL_WENDLAND_C2)
    return Scene(ctx)


# ------------------------------------------------------------------------------------------------------------------------------ lists
def check_lists(S, what):
    h = S.h
    on_particles, repeated, bad = S.groups[1], S.groups[2], S.groups[3]
    for boundary in (False, True):
        for radius in (h, F(h * F(0.9)), F(h * F(0.5)), np.finfo(F).tiny):
            ref = S.ref(radius, boundary)
            dev = S.ctx.query(S.pts, radius, boundary=boundary)
            assert_same(dev, ref, "%s r=%g boundary=%d" % (what, radius, boundary))
            per = np.diff(dev["offsets"].astype(np.int64))
            assert not per[bad].any() and (dev["nearest"][bad] == _lib.QUERY_NONE).all()
            assert (dev["nearest_dist_sq"][bad].view(np.uint32) == _lib.QUERY_NONE_WORD).all()
            assert len(set(per[repeated].tolist())) == 1
            first = int(dev["offsets"][repeated.start])
            for k in range(repeated.start, repeated.stop):  # identical lists
                a = int(dev["offsets"][k])
                assert np.array_equal(dev["index"][a:a + per[k]], dev["index"][first:first + per[k]])
        # FLT_MIN: r2 underflows to 0 — only the points on particles of this set find anything: exactly that particle, at d2 = 0
        tiny = S.ctx.query(S.pts, np.finfo(F).tiny, boundary=boundary)
        per = np.diff(tiny["offsets"].astype(np.int64))
        mine = slice(on_particles.start + (300 if boundary else 0), on_particles.start + (500 if boundary else 300))
        assert per.sum() == per[mine].sum() and (per[mine] >= 1).all() and not tiny["dist_sq"].any()
        src = S.st["boundary"] if boundary else S.st["pos"]
        assert np.array_equal(src[tiny["index"]], np.repeat(S.pts[mine], per[mine], 0))  # (walls that overlap hold particles twice)
        if not boundary:
            assert (per[mine] == 1).all()
    assert S.ref(h, False)["count"] > 10000 and S.ref(h, True)["count"] > 1000


def test_lists_dfsph(dfsph):
    check_lists(dfsph, "dfsph 60 steps")


def test_lists_wcsph(wcsph):
    check_lists(wcsph, "wcsph 60 steps")


def test_lists_after_build_and_densities_only(built):
    check_lists(built, "build + densities")


def test_count_equals_sample_count(dfsph):
    S = dfsph
    got = S.ctx.query(S.pts, None, lists=False, nearest=False)
    assert np.array_equal(np.diff(got["offsets"].astype(np.int64)).astype(np.uint32), S.ctx.sample(S.pts, fields=("count",))["count"])


# ------------------------------------------------------------------------------------------------------------------------------ sizes
@pytest.mark.parametrize("m", [1, 63, 64, 65, 255, 256, 257])
def test_size_edges(dfsph, m):
    S = dfsph
    ref = qr.query32(S.K, S.st, S.pts[:m], S.h)
    assert_same(S.ctx.query(S.pts[:m], S.h), ref, "m=%d" % m)
    assert_same(S.ctx.query(S.pts[:m], S.h, boundary=True), qr.query32(S.K, S.st, S.pts[:m], S.h, True), "m=%d boundary" % m)


def test_more_than_256_workgroups(dfsph):
    """m = 65 537 + 300: 258 workgroups — the carry kernel takes a second chunk"""
    S = dfsph
    m = 65537 + 300
    pts = np.resize(S.pts[S.groups[0]], (m, 2)).astype(F)
    pts[1::2] += F(0.37) * S.h
    ref = qr.query32(S.K, S.st, pts, S.h)
    assert ref["count"] > 300000
    assert_same(S.ctx.query(pts, S.h), ref, "m=%d" % m)


def test_empty_point_set(dfsph):
    S = dfsph
    r = S.ctx.query(np.zeros((0, 2), F))
    assert r["count"] == 0 and r["offsets"].tolist() == [0] and len(r["index"]) == 0
    cnt, off = np.full(1, 7, np.uint64), np.full(1, 7, np.uint64)
    o = _lib.SphxQueryOut(count=cnt.ctypes.data, offsets=off.ctypes.data)
    assert S.ctx.L.sphx_query_radius(S.ctx.h, None, 0, S.h, 0, 0, C.byref(o)) == OK and cnt[0] == 0 and off[0] == 0
    fresh = scene_ctx()  # (an empty set is answered once the arguments pass, whatever the state)
    assert fresh.L.sphx_query_radius(fresh.h, None, 0, S.h, 0, 0, C.byref(o)) == OK


# ------------------------------------------------------------------------------------------------------------------------- dense cell
def test_dense_cell():
    """3 000 particles inside one cell (below the 4 096 of SPHX_FLAG_DENSE_CELL), 300 points in it at radius h: ~900 000 entries"""
    ctx = y.SphxContext()
    K = sr.Constants(ctx.params)
    h = K.h
    rng = np.random.default_rng(3)
    corner = (np.floor((np.array([0.5, 0.5], F) - K.gmin) * K.cell_inv) / K.cell_inv + K.gmin).astype(F)
    pos = (corner + (F(0.3) + F(0.4) * rng.random((3000, 2), dtype=F)) * h).astype(F)
    assert len(np.unique(sr.cells_of(K, pos), axis=0)) == 1
    ctx.set_boundary(np.zeros((0, 2), F))
    ctx.upload(pos)
    ctx.update_neighborhood()
    ctx.update_densities(y.KERNEL_WENDLAND_C2)
    assert not ctx.last_flags() & (y.FLAG_DENSE_CELL | y.FLAG_STRAY_PARTICLES)
    d = ctx.download()
    st = dict(pos=d["pos"], ids=d["ids"], boundary=np.zeros((0, 2), F))
    pts = (corner + (F(0.3) + F(0.4) * rng.random((300, 2), dtype=F)) * h).astype(F)
    ref = qr.query32(K, st, pts, h)
    assert ref["count"] > 850000
    assert_same(ctx.query(pts, h), ref, "dense cell")
    assert ctx.query(pts, h, boundary=True)["count"] == 0  # (no boundary at all: every list is empty)
    # the seam between a workgroup that stages its entries in LDS (<= 4 096 of them) and one that stores them directly: one point (3 000
    # entries), two (6 000), and 257 (a direct workgroup followed by a staged one); a capacity that ends inside either kind
    for m in (1, 2, 257):
        sub = qr.query32(K, st, pts[:m], h)
        assert_same(ctx.query(pts[:m], h), sub, "dense cell, %d points" % m)
        for cap in (1500, sub["count"] - 1500):
            part = ctx.query(pts[:m], h, cap=cap)
            n = min(cap, sub["count"])
            assert part["count"] == sub["count"] and np.array_equal(part["offsets"], sub["offsets"])
            assert np.array_equal(part["index"], sub["index"][:n]) and np.array_equal(part["dist_sq"].view(np.uint32), sub["dist_sq"][:n].view(np.uint32))
            rc, a = raw_query(ctx, np.ascontiguousarray(pts[:m]), h, cap)
            assert rc == OK and all((a[k].view(np.uint32)[n:] == SENTINEL).all() for k in ("index", "id", "dist_sq")), (m, cap)
            assert np.array_equal(a["id"][:n], sub["id"][:n])


# --------------------------------------------------------------------------------------------------------------------------- capacity
def raw_query(ctx, pts, radius, cap, flags=0, lists=True, pad=16):
    """the host-pointer call with sentinel-filled outputs `pad` entries longer than cap -> (rc, arrays)"""
    m = len(pts)
    a = dict(offsets=np.full(m + 1, SENTINEL, np.uint64), count=np.full(1, SENTINEL, np.uint64), nearest=np.full(m, SENTINEL, np.uint32),
             nearest_dist_sq=np.full(m, SENTINEL, np.uint32).view(F))
    if lists:
        a.update(index=np.full(cap + pad, SENTINEL, np.uint32), id=np.full(cap + pad, SENTINEL, np.uint32),
                 dist_sq=np.full(cap + pad, SENTINEL, np.uint32).view(F))
    o = _lib.SphxQueryOut(**{k: v.ctypes.data for k, v in a.items()})
    return ctx.L.sphx_query_radius(ctx.h, pts.ctypes.data_as(C.c_void_p), m, radius, cap, flags, C.byref(o)), a


def test_capacity_and_count_only(dfsph):
    S = dfsph
    ref = S.ref(S.h, False)
    total = ref["count"]
    for cap in (0, total - 1, total, total + 7):
        rc, a = raw_query(S.ctx, S.pts, S.h, cap)
        assert rc == OK and a["count"][0] == total and np.array_equal(a["offsets"], ref["offsets"])
        n = min(cap, total)
        for k in ("index", "id", "dist_sq"):
            got = a[k].view(np.uint32)
            assert np.array_equal(got[:n], np.asarray(ref[k]).view(np.uint32)[:n]) and (got[n:] == SENTINEL).all(), (cap, k)
        assert np.array_equal(a["nearest"], ref["nearest"])
    rc, a = raw_query(S.ctx, S.pts, S.h, total, lists=False)  # count only: all three list pointers NULL
    assert rc == OK and a["count"][0] == total and np.array_equal(a["offsets"], ref["offsets"])
    assert np.array_equal(a["nearest_dist_sq"].view(np.uint32), ref["nearest_dist_sq"].view(np.uint32))
    # the Python method with a capacity returns the prefix
    part = S.ctx.query(S.pts, S.h, cap=1000)
    assert part["count"] == total and len(part["index"]) == 1000 and np.array_equal(part["id"], ref["id"][:1000])


# -------------------------------------------------------------------------------------------------------------------- device pointers
def test_device_pointers_agree_with_the_host_path(dfsph):
    import torch

    S = dfsph
    tp = torch.from_numpy(S.pts).cuda()
    for boundary in (False, True):
        ref = S.ref(S.h, boundary)
        total = ref["count"]
        dev = S.ctx.query(tp, S.h, boundary=boundary)
        assert_same({k: (v.cpu().numpy() if k != "count" else v) for k, v in dev.items()}, ref, "device boundary=%d" % boundary)
        # sentinel behind the capacity, twice: identical bytes
        runs = []
        for _ in range(2):
            out = dict(index=torch.full((total + 9,), -3, dtype=torch.int32, device="cuda"), id=torch.full((total + 9,), -3, dtype=torch.int32, device="cuda"),
                       dist_sq=torch.full((total + 9,), -3.0, device="cuda"), offsets=torch.full((len(S.pts) + 1,), -3, dtype=torch.int64, device="cuda"),
                       nearest=torch.full((len(S.pts),), -3, dtype=torch.int32, device="cuda"), count=torch.full((1,), -3, dtype=torch.int64, device="cuda"))
            r = S.ctx.query(tp, S.h, boundary=boundary, cap=total - 5, out=out)
            assert r["count"] == total and len(r["index"]) == total - 5
            assert (out["index"][total - 5:] == -3).all() and (out["id"][total - 5:] == -3).all() and (out["dist_sq"][total - 5:] == -3.0).all()
            runs.append(b"".join(out[k].cpu().numpy().tobytes() for k in sorted(out)))
            assert np.array_equal(out["index"][:total - 5].cpu().numpy().astype(np.uint32), ref["index"][:total - 5])
            assert np.array_equal(out["offsets"].cpu().numpy().astype(np.uint64), ref["offsets"])
        assert runs[0] == runs[1]
        # count only on the device path, without offsets of the caller's
        cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
        o = _lib.SphxQueryOut(count=cnt.data_ptr())
        flags = _lib.QUERY_DEVICE_POINTERS | (_lib.QUERY_BOUNDARY if boundary else 0)
        torch.cuda.synchronize()
        assert S.ctx.L.sphx_query_radius(S.ctx.h, C.c_void_p(tp.data_ptr()), len(S.pts), S.h, 0, flags, C.byref(o)) == OK
        S.ctx.synchronize()
        assert int(cnt.item()) == total
        # lists without offsets of the caller's
        idx = torch.full((total,), -3, dtype=torch.int32, device="cuda")
        o = _lib.SphxQueryOut(count=cnt.data_ptr(), index=idx.data_ptr())
        assert S.ctx.L.sphx_query_radius(S.ctx.h, C.c_void_p(tp.data_ptr()), len(S.pts), S.h, total, flags, C.byref(o)) == OK
        S.ctx.synchronize()
        assert np.array_equal(idx.cpu().numpy().astype(np.uint32), ref["index"])


# ------------------------------------------------------------------------------------------------------- state rules, argument errors
def _q(ctx, radius=0.02, m=4, xy=None, flags=0, out=None, cap=0):
    cnt = np.zeros(1, np.uint64)
    o = _lib.SphxQueryOut(count=cnt.ctypes.data) if out is None else out
    pts = np.full((4, 2), 0.5, F) if xy is None else xy
    return ctx.L.sphx_query_radius(ctx.h, None if pts is False else pts.ctypes.data_as(C.c_void_p), m, radius, cap, flags, C.byref(o) if o else None)


def _s(ctx, rects=((0.0, 0.0, 1.0, 1.0),), flags=0, out=None, n=None):
    cnt = np.zeros(1, np.uint32)
    o = _lib.SphxSelectOut(count=cnt.ctypes.data) if out is None else out
    arr, k = y._rect_array(rects)
    return ctx.L.sphx_select(ctx.h, arr, k if n is None else n, flags, 0, C.byref(o) if o else None)


def err(ctx):
    return ctx.L.sphx_last_error(ctx.h).decode()


def test_state_rules():
    ctx = scene_ctx()
    assert _q(ctx) == E_READY and "sphx_upload" in err(ctx)
    assert _s(ctx) == OK  # (wherever sphx_download is allowed)
    ctx.update_neighborhood()
    assert _q(ctx) == E_READY and "sphx_update_densities" in err(ctx)
    ctx.update_densities(y.KERNEL_WENDLAND_C2)
    assert _q(ctx) == OK
    ctx.set_boundary(ctx.download_boundary()[0])
    assert _q(ctx) == E_READY and "sphx_set_boundary" in err(ctx)
    timer = y.TimeManager()
    dfsph_steps(ctx, timer, 2)
    assert _q(ctx) == OK and _q(ctx, flags=_lib.QUERY_BOUNDARY) == OK
    blob = ctx.save_state()
    first = ctx.append(np.array([[0.3, 1.5]], F))
    assert _q(ctx) == E_READY and "sphx_append" in err(ctx) and _s(ctx) == OK
    dfsph_steps(ctx, timer, 1)
    assert _q(ctx) == OK
    assert ctx.remove([(5.0, 5.0, 6.0, 6.0)]) == 0 and _q(ctx) == OK  # (nothing removed: the context is untouched)
    assert ctx.remove([(0.29, 1.0, 0.31, 2.0)]) >= 1 and first > 0
    assert _q(ctx) == E_READY and "sphx_remove" in err(ctx)
    dfsph_steps(ctx, timer, 1)
    ctx.step_begin(timer.simulation_step())
    assert _q(ctx) == E_READY and _s(ctx) == E_READY and "step" in err(ctx)
    ctx.step_finish(y.duration_as_secs_f32(timer.update_simulation_step(DIAM, 0.0)))
    assert _q(ctx) == OK and _s(ctx) == OK
    ctx.step_begin(timer.simulation_step())
    with pytest.raises(y.SphxError):
        ctx.step_finish(-1.0)  # a failed step
    assert _q(ctx) == E_READY
    other = y.SphxContext()
    other.load_state(blob)  # a ready state: allowed at once
    assert _q(other) == OK and _s(other) == OK
    # tile contexts are refused
    tc = scene_ctx()
    assert tc.L.sphx_tile_configure(tc.h, 0, 0, 65536, 4, 0, 0) == OK
    assert _q(tc) == E_ARG and "tile" in err(tc) and _s(tc) == E_ARG and "tile" in err(tc)
    from yasph2d_amd.multi import MultiSolver

    pos, bnd = dam_break()
    m = MultiSolver(y.default_params(), devices=[0, 0])
    m.set_boundary(bnd)
    m.upload(pos)
    t = m.tile_context(0)
    assert _q(t) == E_ARG and "tile" in err(t) and _s(t) == E_ARG and "tile" in err(t)


def test_argument_errors(dfsph):
    ctx = dfsph.ctx
    h = dfsph.h
    assert _q(ctx, radius=h) == OK
    for bad in (0.0, -0.01, float("nan"), float("inf"), np.nextafter(h, F(np.inf))):
        assert _q(ctx, radius=bad) == E_ARG and "radius" in err(ctx), bad
    assert ctx.L.sphx_query_radius(None, None, 0, h, 0, 0, None) == E_ARG
    assert _q(ctx, out=False) == E_ARG and "out" in err(ctx)
    assert _q(ctx, out=_lib.SphxQueryOut()) == E_ARG and "count" in err(ctx)
    assert _q(ctx, xy=False) == E_ARG and "xy" in err(ctx)
    assert _q(ctx, flags=4) == E_ARG and "flags" in err(ctx) and _q(ctx, flags=0x80000000) == E_ARG
    assert _q(ctx, m=1 << 31) == E_ARG and "m " in err(ctx)
    import torch

    buf = torch.zeros(8, dtype=torch.int32, device="cuda")
    pts = torch.full((4, 2), 0.5, device="cuda")
    for o, name in ((_lib.SphxQueryOut(count=buf.data_ptr() + 4), "count"), (_lib.SphxQueryOut(count=buf.data_ptr(), offsets=buf.data_ptr() + 4), "offsets")):
        rc = ctx.L.sphx_query_radius(ctx.h, C.c_void_p(pts.data_ptr()), 4, h, 0, _lib.QUERY_DEVICE_POINTERS, C.byref(o))
        assert rc == E_ARG and name in err(ctx) and "aligned" in err(ctx)
    for bad in (np.zeros((4, 3), F), np.zeros(8, F)):
        with pytest.raises(ValueError):
            ctx.query(bad)
    # sphx_select
    assert ctx.L.sphx_select(None, None, 0, 0, 0, None) == E_ARG
    assert _s(ctx, out=False) == E_ARG and "out" in err(ctx)
    assert _s(ctx, out=_lib.SphxSelectOut()) == E_ARG and "count" in err(ctx)
    assert _s(ctx, flags=4) == E_ARG and "flags" in err(ctx)
    assert _s(ctx, rects=[(0.0, 0.0, float("nan"), 1.0)]) == E_ARG and "rect" in err(ctx)
    assert _s(ctx, rects=[(0.0, 0.0, 1.0, 1.0)] * 9) == E_ARG and "n_rects" in err(ctx)
    cnt = np.zeros(1, np.uint32)
    assert ctx.L.sphx_select(ctx.h, None, 2, 0, 0, C.byref(_lib.SphxSelectOut(count=cnt.ctypes.data))) == E_ARG and "rects" in err(ctx)


# --------------------------------------------------------------------------------------------------------------------- no side effects
def test_queries_and_selects_have_no_side_effects():
    def run(query):
        ctx = scene_ctx()
        timer = y.TimeManager()
        pts = (np.array([0.0, 0.4]) + np.random.default_rng(5).random((700, 2)) * np.array([0.8, 1.4])).astype(F)
        stats = []
        for _ in range(40):
            vmax = ctx.step_begin(timer.simulation_step(), timer.law(DIAM))
            stats.append(ctx.step_finish(y.duration_as_secs_f32(timer.update_simulation_step(DIAM, vmax))))
            if query:
                assert ctx.query(pts)["count"] > 0
                ctx.query(pts, boundary=True, lists=False)
                assert ctx.select([(0.0, 0.5, 0.4, 1.2)])["count"] > 0
        return ctx.state_digest(), stats, ctx.last_flags(), timer.simulation_step_ns()

    assert run(True) == run(False)


# ----------------------------------------------------------------------------------------------------------------------------- select
RECT_CASES = [
    ("one", [(0.1, 0.7, 0.4, 1.2)], False),
    ("eight overlapping", [(0.1 + 0.03 * k, 0.7 + 0.05 * k, 0.3 + 0.03 * k, 1.0 + 0.05 * k) for k in range(8)], False),
    ("empty", [(0.4, 0.7, 0.1, 1.2)], False),
    ("half planes", [(-np.inf, -np.inf, 0.3, np.inf), (-np.inf, 1.4, np.inf, np.inf)], False),
    ("outside", [(0.1, 0.7, 0.4, 1.2), (0.3, 0.9, 0.6, 1.5)], True),
    ("none", [], False),
    ("none outside", [], True),
]


@pytest.fixture(scope="module")
def nan_scene():
    """the dam break as uploaded, with NaN particles among it (in no rectangle; selected by `outside`): sphx_select needs no build"""
    pos, bnd = dam_break()
    pos = np.concatenate([pos[:1000], np.array([[np.nan, 0.2], [0.2, np.nan]], F), pos[1000:]]).astype(F)
    ctx = y.SphxContext()
    ctx.set_boundary(bnd)
    ctx.upload(pos)
    d = ctx.download()
    assert np.isnan(d["pos"]).any()
    return ctx, d


@pytest.mark.parametrize("what,rects,outside", RECT_CASES, ids=[c[0] for c in RECT_CASES])
def test_select_equals_reference(nan_scene, what, rects, outside):
    import torch

    ctx, d = nan_scene
    ref = qr.select32(d["pos"], d["ids"], rects, outside)
    nan_slot = int(np.nonzero(np.isnan(d["pos"][:, 0]))[0][0])
    assert (nan_slot in ref["index"].tolist()) == outside
    got = ctx.select(rects, outside)
    assert got["count"] == ref["count"] and np.array_equal(got["index"], ref["index"]) and np.array_equal(got["id"], ref["id"])
    total = ref["count"]
    for cap in sorted({0, max(total - 1, 0), total, total + 7}):
        idx, ids, cnt = np.full(cap + 8, SENTINEL, np.uint32), np.full(cap + 8, SENTINEL, np.uint32), np.full(1, SENTINEL, np.uint32)
        arr, k = y._rect_array(rects)
        o = _lib.SphxSelectOut(index=idx.ctypes.data, id=ids.ctypes.data, count=cnt.ctypes.data)
        assert ctx.L.sphx_select(ctx.h, arr, k, _lib.SELECT_OUTSIDE if outside else 0, cap, C.byref(o)) == OK
        n = min(cap, total)
        assert cnt[0] == total and np.array_equal(idx[:n], ref["index"][:n]) and np.array_equal(ids[:n], ref["id"][:n])
        assert (idx[n:] == SENTINEL).all() and (ids[n:] == SENTINEL).all()
        out = dict(index=torch.full((cap + 8,), -3, dtype=torch.int32, device="cuda"), id=torch.full((cap + 8,), -3, dtype=torch.int32, device="cuda"))
        r = ctx.select(rects, outside, cap=cap, out=out)
        assert r["count"] == total and np.array_equal(out["index"].cpu().numpy().view(np.uint32)[:n], ref["index"][:n])
        assert np.array_equal(out["id"].cpu().numpy().view(np.uint32)[:n], ref["id"][:n])
        assert (out["index"][n:] == -3).all() and (out["id"][n:] == -3).all()


def test_select_ties_to_remove_and_track(dfsph):
    ctx = dfsph.ctx
    lo, hi = dfsph.st["pos"].min(0), dfsph.st["pos"].max(0)
    mid = F(0.5) * (lo + hi)
    rects = [(lo[0], lo[1], mid[0], mid[1]), (mid[0] - F(0.05), mid[1] - F(0.05), hi[0], F(0.25) * lo[1] + F(0.75) * hi[1])]
    sel = ctx.select(rects)
    assert 100 < sel["count"] < ctx.n
    other = y.SphxContext()
    other.load_state(ctx.save_state())
    assert other.remove(rects) == sel["count"]
    kept = other.download()["ids"]
    assert np.array_equal(np.sort(np.concatenate([kept, sel["id"]])), np.sort(dfsph.st["ids"])) and not np.intersect1d(kept, sel["id"]).size
    ctx.track(sel["id"])
    assert np.array_equal(ctx.track_fetch()["slot"], sel["index"])
    ctx.track([])
    # picking: the nearest particle to a point, then followed by id
    q = ctx.query(dfsph.pts[:8], nearest=True)
    hit = q["nearest"] != _lib.QUERY_NONE
    assert hit.any()
    ctx.track(dfsph.st["ids"][q["nearest"][hit]])
    assert np.array_equal(ctx.track_fetch()["slot"], q["nearest"][hit])
    ctx.track([])


# ---------------------------------------------------------------------------------------------------------------------------- harness
def test_harness_csvs_match_python(tmp_path):
    steps = 12
    pts = [(0.3, 1.0), (0.5, 1.2), (1.7, 0.9), (0.2, 0.75)]
    rect = (0.1, 0.6, 0.45, 1.3)
    qp, sp = tmp_path / "query.csv", tmp_path / "select.csv"
    out = subprocess.run([HARNESS, "--scale", "1", "--steps", str(steps), "--warmup", "0", "--query-out", str(qp), "--query-points",
                          ";".join("%r,%r" % p for p in pts), "--query-radius", "0.018", "--select-out", str(sp), "--select", ",".join(map(str, rect))],
                         capture_output=True, text=True, timeout=300)
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
    q = ctx.query(np.array(pts, F), F(0.018))
    rows = open(qp).read().splitlines()
    assert rows[0] == "point,slot,id,dist_sq" and len(rows) - 1 == q["count"] > 10
    got = np.array([[float(v) for v in r.split(",")] for r in rows[1:]])
    point = np.repeat(np.arange(len(pts)), np.diff(q["offsets"].astype(np.int64)))
    assert np.array_equal(got[:, 0], point) and np.array_equal(got[:, 1], q["index"]) and np.array_equal(got[:, 2], q["id"])
    assert np.array_equal(got[:, 3].astype(F).view(np.uint32), q["dist_sq"].view(np.uint32))
    s = ctx.select([rect])
    rows = open(sp).read().splitlines()
    assert rows[0] == "slot,id" and len(rows) - 1 == s["count"] > 100
    got = np.array([[int(v) for v in r.split(",")] for r in rows[1:]])
    assert np.array_equal(got[:, 0], s["index"]) and np.array_equal(got[:, 1], s["id"])
    assert '"query_entries": %d' % q["count"] in out.stdout and '"selected": %d' % s["count"] in out.stdout
    for bad in (["--query-out", str(qp)], ["--query-points", "0,0"], ["--query-out", str(qp), "--query-points", "0,0;1"],
                ["--query-out", str(qp), "--query-points", "0,0", "--query-radius", "0"], ["--select-out", str(sp)], ["--select", "0,0,1,1"],
                ["--select-out", str(sp), "--select", "0,0,1"]):
        r = subprocess.run([HARNESS, "--scale", "1", "--steps", "1", "--warmup", "0"] + bad, capture_output=True, text=True, timeout=120)
        assert r.returncode == 2, bad
