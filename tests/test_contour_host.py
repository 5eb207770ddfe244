"""Free-surface extraction without a GPU: the C ABI exports sphx_surface_contour and sphx_contour_chain; the numpy restatement of the
contour contract (tests/contour_reference.py), which the GPU tests hold the device to bit for bit, is itself checked on hand-made
lattices and on a sampled scene; sphx_contour_chain (plain host code) is compared with the Python restatement of its rule."""
import ctypes as C

import numpy as np
import pytest

import contour_reference as cr
import sample_reference as sr
import yasph2d_amd as y
from util import uniform_points
from yasph2d_amd import _lib

F = np.float32
B, R, T, L = cr.EDGE_B, cr.EDGE_R, cr.EDGE_T, cr.EDGE_L


def test_contour_symbols_exported_and_null_context_rejected(sphx_lib):
    for name in ("sphx_surface_contour", "sphx_contour_chain"):
        assert hasattr(sphx_lib, name) and name in _lib.SIGNATURES
    cnt = np.zeros(1, np.uint32)
    out = _lib.SphxContourOut(count=cnt.ctypes.data)
    assert sphx_lib.sphx_surface_contour(None, 0.0, 0.0, 0.1, 0.1, 2, 2, 0, 0, 0.5, 0, 0, C.byref(out)) == _lib.ERR_INVALID_ARGUMENT
    assert C.sizeof(_lib.SphxContourOut) == 4 * C.sizeof(C.c_void_p)
    assert callable(y.contour_lines) and callable(y.contour_chain) and hasattr(y.SphxContext, "contour")


# ------------------------------------------------------------------------------------------------------------- hand-made lattices
X0, Y0, DX, DY = F(0.25), F(-1.5), F(0.125), F(0.5)  # (exact in fp32: the expected points below are plain arithmetic)


def _one_cell(f0, f1, f2, f3, iso=0.5):
    return cr.contour32(np.array([[f0, f1], [f3, f2]], F), X0, Y0, DX, DY, 2, 2, iso)


def _edge_point(e, f, iso=F(0.5)):
    """the contract's crossing, written out scalar by scalar"""
    xl, xr, yb, yt = X0, F(X0 + DX), Y0, F(Y0 + DY)
    xa, ya, xb, yb_, fa, fb = {B: (xl, yb, xr, yb, f[0], f[1]), R: (xr, yb, xr, yt, f[1], f[2]), T: (xl, yt, xr, yt, f[3], f[2]),
                               L: (xl, yb, xl, yt, f[0], f[3])}[e]
    t = F(F(iso - fa) / F(fb - fa))
    return np.array([F(xa + F(t * F(xb - xa))), F(ya + F(t * F(yb_ - ya)))], F)


@pytest.mark.parametrize("case", range(16))
def test_one_cell_per_case(case):
    inside, outside = F(0.875), F(0.25)
    f = [inside if case >> k & 1 else outside for k in range(4)]
    r = _one_cell(*f)
    assert r["case"][0] == case
    if case in (0, 15):
        assert r["count"] == 0
        return
    if case in (5, 10):
        # centre = (0.875 + 0.25 + 0.875 + 0.25) / 4 = 0.5625 >= 0.5: inside
        assert r["centre_inside"][0]
        want = cr.SADDLES[case][0]
    else:
        want = cr.SEGMENTS[case]
    assert r["count"] == len(want) and (r["cell"] == 0).all()
    for k, (a, b) in enumerate(want):
        assert np.array_equal(r["segments"][k, 0], _edge_point(a, f)) and np.array_equal(r["segments"][k, 1], _edge_point(b, f))
        # inside on the left: the cross product of the direction with (an inside node - start) is positive
        d = r["segments"][k, 1].astype(np.float64) - r["segments"][k, 0]
        nodes = np.array([[X0, Y0], [X0 + DX, Y0], [X0 + DX, Y0 + DY], [X0, Y0 + DY]], np.float64)
        for node in range(4):
            side = d[0] * (nodes[node, 1] - r["segments"][k, 0, 1]) - d[1] * (nodes[node, 0] - r["segments"][k, 0, 0])
            if case not in (5, 10):
                assert (side > 0) == bool(case >> node & 1), (case, node)
    # the order inside a saddle cell: the segment that starts on the earlier edge (B, R, T, L) first
    if len(want) == 2:
        assert want[0][0] < want[1][0]


def test_both_saddle_resolutions():
    for case, (hi, lo) in ((5, (0.875, 0.25)), (10, (0.875, 0.25))):
        for centre_in, low in ((True, lo), (False, 0.0)):  # (0.875 + 0 + 0.875 + 0) / 4 = 0.4375 < 0.5: outside
            f = [F(hi) if case >> k & 1 else F(low) for k in range(4)]
            r = _one_cell(*f)
            want = cr.SADDLES[case][0 if centre_in else 1]
            assert r["count"] == 2 and bool(r["centre_inside"][0]) == centre_in
            for k, (a, b) in enumerate(want):
                assert np.array_equal(r["segments"][k, 0], _edge_point(a, f)) and np.array_equal(r["segments"][k, 1], _edge_point(b, f))
    # the four resolutions' tables are the contract's
    assert cr.SADDLES[5] == ([(B, R), (T, L)], [(B, L), (T, R)]) and cr.SADDLES[10] == ([(R, T), (L, B)], [(R, B), (L, T)])
    # the centre is ((f0 + f1) + (f2 + f3)) * 0.25f in fp32: a lattice where the pairing decides
    f = [F(1.0), F(2.0 ** -25), F(1.0), F(2.0 ** -25)]  # (1 + 2^-25) rounds to 1: centre = 0.5 exactly -> inside at iso 0.5
    assert _one_cell(*f)["centre_inside"][0]
    assert not _one_cell(*f, iso=np.nextafter(F(0.5), F(1)))["centre_inside"][0]


def test_value_equal_to_iso_is_inside_and_nan_is_outside():
    # f == iso exactly on node 0: inside; the crossings of its edges sit on the node itself (t = 0)
    r = _one_cell(F(0.5), F(0.25), F(0.125), F(0.25))
    assert r["case"][0] == 1 and r["count"] == 1
    assert np.array_equal(r["segments"][0], np.array([[X0, Y0], [X0, Y0]], F))
    # a NaN node is outside whatever its neighbours are
    r = _one_cell(F(np.nan), F(1.0), F(1.0), F(1.0))
    assert r["case"][0] == 14 and r["count"] == 1 and np.isnan(r["segments"][0]).any()
    r = _one_cell(F(np.nan), F(np.nan), F(np.nan), F(np.nan))
    assert r["case"][0] == 0 and r["count"] == 0
    # infinities compare as numbers
    assert _one_cell(F(np.inf), F(-np.inf), F(0.0), F(0.0))["case"][0] == 1
    # nx < 2 or ny < 2: no cell
    assert cr.contour32(np.ones(5, F), 0, 0, 1, 1, 5, 1, 0.5)["count"] == 0 and cr.contour32(np.ones(5, F), 0, 0, 1, 1, 1, 5, 0.5)["count"] == 0


def test_shared_edges_give_the_same_bits_and_the_order_is_by_cell():
    rng = np.random.default_rng(5)
    nx, ny = 23, 17
    f = rng.random((ny, nx), dtype=F)
    r = cr.contour32(f, F(0.1), F(0.2), F(0.013), F(0.017), nx, ny, 0.5)
    assert r["count"] > 100 and set(np.unique(r["case"])) == set(range(16))
    assert (np.diff(r["cell"].astype(np.int64)) >= 0).all()
    # every end point strictly inside the lattice is some segment's start, bit for bit (the neighbouring cell computed it again)
    xs = F(0.1) + np.arange(nx, dtype=F) * F(0.013)
    ys = F(0.2) + np.arange(ny, dtype=F) * F(0.017)
    seg = r["segments"]
    starts = {p.tobytes() for p in seg[:, 0]}
    interior = lambda p: xs[0] < p[0] < xs[-1] and ys[0] < p[1] < ys[-1]
    assert all(p.tobytes() in starts for p in seg[:, 1] if interior(p))
    # ... and per cell the count is that of its case
    per_cell = np.bincount(r["cell"], minlength=(nx - 1) * (ny - 1))
    want = np.where((r["case"] == 0) | (r["case"] == 15), 0, np.where((r["case"] == 5) | (r["case"] == 10), 2, 1))
    assert np.array_equal(per_cell, want)


# ------------------------------------------------------------------------------------------------------------- a sampled scene
SPRAY_LATTICE = (F(0.27), F(0.27), F(0.0119), F(0.0131), 50, 46)


def _spray_values():
    """700 scattered particles, densities from the restated sampling at the particles (clamped like the solver's), fraction on a lattice
    that surrounds the fluid by more than h"""
    K = sr.Constants(y.default_params())
    pos = (uniform_points(700, 2500.0, 11) + F(0.3)).astype(F)
    st = dict(pos=pos, vel=np.zeros_like(pos), density=np.zeros(len(pos), F), boundary=np.zeros((0, 2), F))
    st["density"] = np.maximum(sr.sample32(K, dict(st, density=np.ones(len(pos), F)), pos, sr.KERNEL_WENDLAND)["density"], K.rho0)
    x0, y0, dx, dy, nx, ny = SPRAY_LATTICE
    assert x0 + float(K.h) < pos[:, 0].min() and pos[:, 0].max() + float(K.h) < x0 + (nx - 1) * dx
    assert y0 + float(K.h) < pos[:, 1].min() and pos[:, 1].max() + float(K.h) < y0 + (ny - 1) * dy
    return sr.sample32(K, st, sr.lattice_points(x0, y0, dx, dy, nx, ny), sr.KERNEL_WENDLAND)["fraction"]


@pytest.fixture(scope="module")
def spray():
    f = _spray_values()
    return f, {iso: cr.contour32(f, *SPRAY_LATTICE, iso) for iso in (0.4, 0.5, 0.6)}


def test_sampled_scene_is_watertight_oriented_and_monotone(spray):
    f, by_iso = spray
    r = by_iso[0.5]
    assert r["count"] > 300 and set(np.unique(r["case"])) == set(range(16))
    assert cr.dangling(r["segments"]) == (0, 0)  # every end is some segment's start and vice versa
    lines, closed = cr.lines_of(r["segments"])
    assert all(closed) and sum(len(l) - 1 for l in lines) == r["count"]
    area = {iso: cr.enclosed_area(v["segments"]) for iso, v in by_iso.items()}
    assert area[0.5] > 0  # inside on the left
    assert area[0.6] < area[0.5] < area[0.4], area  # a higher threshold encloses less
    # the enclosed region holds every cell whose four nodes are inside and lies within the cells that have an inside node
    x0, y0, dx, dy, nx, ny = SPRAY_LATTICE
    cell_area = float(dx) * float(dy)
    full, touched = int((r["case"] == 15).sum()), int((r["case"] != 0).sum())
    assert full * cell_area < area[0.5] < touched * cell_area, (area[0.5], full * cell_area, touched * cell_area)


# ------------------------------------------------------------------------------------------------------------- sphx_contour_chain
def _chain_lib(lib, seg):
    seg = np.ascontiguousarray(seg, F).reshape(-1, 4)
    n = len(seg)
    order, first, closed, lines = np.full(n, 0xFFFFFFFF, np.uint32), np.full(n + 1, 0xFFFFFFFF, np.uint32), np.full(n, 7, np.uint8), C.c_uint32(99)
    rc = lib.sphx_contour_chain(seg.ctypes.data_as(C.c_void_p), n, order.ctypes.data_as(C.c_void_p), first.ctypes.data_as(C.c_void_p),
                                closed.ctypes.data_as(C.c_void_p), C.byref(lines))
    assert rc == _lib.OK
    return order, first[:lines.value + 1], closed[:lines.value].astype(bool)


def _same_chain(lib, seg):
    a, b = _chain_lib(lib, seg), cr.chain(seg)
    for u, v in zip(a, b):
        assert np.array_equal(u, v)
    order, first, closed = a
    assert sorted(order.tolist()) == list(range(len(order))) and first[-1] == len(order) and (np.diff(first.astype(np.int64)) > 0).all()
    # every line is a chain: each segment starts where its predecessor ends
    s = np.asarray(seg, F).reshape(-1, 2, 2)
    for k in range(len(closed)):
        idx = order[first[k]:first[k + 1]]
        assert np.array_equal(s[idx[1:], 0], s[idx[:-1], 1])
        assert closed[k] == 0 or np.array_equal(s[idx[0], 0], s[idx[-1], 1])
    return a


def test_chain_matches_the_restatement(sphx_lib, spray):
    seg = spray[1][0.5]["segments"]
    order, first, closed = _same_chain(sphx_lib, seg)
    assert closed.all() and len(closed) > 3
    # a shuffled copy: the same lines as point sets, found from other first segments
    rng = np.random.default_rng(3)
    perm = rng.permutation(len(seg))
    o2, f2, c2 = _same_chain(sphx_lib, seg[perm])
    assert c2.all() and len(c2) == len(closed)
    assert sorted(len(x) for x in np.split(o2, f2[1:-1])) == sorted(len(x) for x in np.split(order, first[1:-1]))
    # the Python wrapper returns the same, as polylines
    lines, cl = y.contour_lines(seg)
    ref_lines, ref_cl = cr.lines_of(seg)
    assert cl == [bool(c) for c in ref_cl] and all(np.array_equal(a, b) for a, b in zip(lines, ref_lines)) and len(lines) == len(ref_lines)


def test_chain_open_lines_nan_and_empty(sphx_lib, spray):
    f, _ = spray
    # the lattice cut off in the middle of the fluid: lines end on the border
    x0, y0, dx, dy, nx, ny = SPRAY_LATTICE
    sub = np.ascontiguousarray(f.reshape(ny, nx)[8:30, 10:33])
    r = cr.contour32(sub, F(x0 + F(10) * dx), F(y0 + F(8) * dy), dx, dy, 23, 22, 0.5)
    assert cr.dangling(r["segments"])[0] > 0
    order, first, closed = _same_chain(sphx_lib, r["segments"])
    assert (~closed).any()
    opened = [k for k in range(len(closed)) if not closed[k]]
    # pass 1 comes first: every open line precedes every closed one, and an open line starts at a point that is nobody's end
    assert opened == list(range(len(opened)))
    ends = {p.tobytes() for p in r["segments"][:, 1]}
    assert all(r["segments"][order[first[k]], 0].tobytes() not in ends for k in opened)
    _same_chain(sphx_lib, r["segments"][np.random.default_rng(9).permutation(r["count"])])
    # segments with NaN: a NaN point equals nothing, not even itself
    seg = r["segments"].copy()
    seg[3, 1, 0] = np.nan
    seg[11, 0, 1] = np.nan
    seg[12] = np.nan
    _same_chain(sphx_lib, seg)
    nan_loop = np.array([[[np.nan, 0], [np.nan, 0]]], F)  # start "equals" end only bitwise
    o, fi, cl = _same_chain(sphx_lib, nan_loop)
    assert len(cl) == 1 and not cl[0]
    # -0 equals +0; duplicates: the lowest unused index follows
    seg = np.array([[[0, 0], [1, 0]], [[1, 0], [1, 1]], [[1, 0], [2, 2]], [[1, 1], [-0.0, 0.0]], [[5, 5], [5, 5]]], F)
    o, fi, cl = _same_chain(sphx_lib, seg)
    # (no start is nobody's end: pass 1 opens nothing; 0 -> 1 (not 2) -> 3 closes through -0 == +0; 2 is left over and open)
    assert o.tolist() == [0, 1, 3, 2, 4] and fi.tolist() == [0, 3, 4, 5] and cl.tolist() == [True, False, True]
    # n = 0, and NULL pointers
    lines = C.c_uint32(5)
    assert sphx_lib.sphx_contour_chain(None, 0, None, None, None, C.byref(lines)) == _lib.OK and lines.value == 0
    assert sphx_lib.sphx_contour_chain(None, 0, None, None, None, None) == _lib.ERR_INVALID_ARGUMENT
    s = np.zeros((2, 4), F)
    buf = np.zeros(4, np.uint32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    for args in ((None, 2, p(buf), p(buf), p(buf)), (p(s), 2, None, p(buf), p(buf)), (p(s), 2, p(buf), None, p(buf)), (p(s), 2, p(buf), p(buf), None)):
        assert sphx_lib.sphx_contour_chain(*args, C.byref(lines)) == _lib.ERR_INVALID_ARGUMENT
    o, fi, cl = y.contour_chain(np.zeros((0, 2, 2), F))
    assert len(o) == 0 and fi.tolist() == [0] and len(cl) == 0 and y.contour_lines(np.zeros((0, 2, 2), F)) == ([], [])


def test_chain_is_not_quadratic(sphx_lib):
    """200 000 segments of one long open line given backwards, plus a many-fold start point: well under a second when the successor
    search is a table look-up (a scan per segment would take minutes)"""
    import time

    n = 200000
    x = np.arange(n + 1, dtype=F)
    seg = np.stack([x[:-1], np.zeros(n, F), x[1:], np.zeros(n, F)], -1)[::-1].copy()
    fan = np.tile(np.array([[-1.0, -1.0, -2.0, -2.0]], F), (20000, 1))  # 20 000 segments that all start at one point
    t0 = time.perf_counter()
    order, first, closed = _chain_lib(sphx_lib, np.concatenate([seg, fan]))
    dt = time.perf_counter() - t0
    assert first.tolist()[:2] == [0, n] and order[0] == n - 1 and order[n - 1] == 0 and len(closed) == 1 + 20000 and not closed.any()
    assert dt < 5.0, dt
