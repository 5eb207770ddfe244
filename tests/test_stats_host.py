"""Fluid statistics without a GPU: the C ABI exports the calls and checks their context argument, the ctypes structs and the numpy dtype
have the layout of include/sphx.h, and the numpy restatement (tests/stats_reference.py), which the GPU tests compare the device with, is
itself checked against hand-made cases."""
import ctypes as C
import math

import numpy as np

import stats_reference as ref
import yasph2d_amd as y
from yasph2d_amd import _lib

F = np.float32
INF = float("inf")


def test_symbols_exported_and_null_context_rejected(sphx_lib):
    for name in ("sphx_fluid_stats", "sphx_stats_record", "sphx_stats_get_status", "sphx_stats_read"):
        assert hasattr(sphx_lib, name) and name in _lib.SIGNATURES, name
    rec = np.zeros(1, y.STATS_DTYPE)
    st = _lib.SphxStatsStatus()
    bad = _lib.ERR_INVALID_ARGUMENT
    assert sphx_lib.sphx_fluid_stats(None, None, 0, 0, rec.ctypes.data) == bad
    assert sphx_lib.sphx_stats_record(None, None, 0, 4, 1) == bad
    assert sphx_lib.sphx_stats_get_status(None, C.byref(st)) == bad
    assert sphx_lib.sphx_stats_read(None, 0, 0, rec.ctypes.data, None) == bad
    assert _lib.STATS_DEVICE_POINTERS == 1 and _lib.STATS_MAX_RECTS == 8
    for method in ("stats", "stats_record", "stats_status", "stats_frames"):
        assert hasattr(y.SphxContext, method), method


def test_struct_layouts():
    offsets = dict(count=0, nonfinite=8, density_count=16, density_valid=24, reserved=28, sum_pos=32, sum_vel=48, sum_speed_sq=64,
                   sum_angular=72, sum_density=80, sum_density_sq=88, max_speed_sq=96, min_pos=104, max_pos=112, min_density=120,
                   max_density=124)
    assert C.sizeof(_lib.SphxStatsRec) == 128 and y.STATS_DTYPE.itemsize == 128
    assert [n for n, _ in _lib.SphxStatsRec._fields_] == list(offsets) == list(y.STATS_DTYPE.names)
    for name, off in offsets.items():
        assert getattr(_lib.SphxStatsRec, name).offset == off, name
        assert y.STATS_DTYPE.fields[name][1] == off, name
        assert getattr(_lib.SphxStatsRec, name).size == y.STATS_DTYPE.fields[name][0].itemsize, name
    assert C.sizeof(_lib.SphxStatsFrame) == 16 and y.STATS_FRAME_DTYPE.itemsize == 16
    for name, off in dict(step=0, dt=8, n=12).items():
        assert getattr(_lib.SphxStatsFrame, name).offset == off and y.STATS_FRAME_DTYPE.fields[name][1] == off, name
    assert C.sizeof(_lib.SphxStatsStatus) == 32
    assert [(n, getattr(_lib.SphxStatsStatus, n).offset) for n, _ in _lib.SphxStatsStatus._fields_] == [
        ("n_rects", 0), ("recording", 4), ("max_frames", 8), ("every", 12), ("frames", 16), ("dropped", 20), ("reserved", 24)]
    assert C.sizeof(_lib.SphxRect) == 16


def as_struct(r):
    """a reference record as one element of STATS_DTYPE (what a device that computed the exact sums would return)"""
    a = np.zeros(1, y.STATS_DTYPE)
    for k in y.STATS_DTYPE.names:
        a[0][k] = r[k]
    return a[0]


def test_empty_set():
    (r,) = ref.stats((np.zeros((0, 2), F), np.zeros((0, 2), F), np.zeros(0, F)))
    assert r["count"] == r["nonfinite"] == r["density_count"] == 0 and r["density_valid"] == 1
    assert r["sum_pos"].tolist() == [0, 0] and r["sum_speed_sq"] == 0 and r["max_speed_sq"] == 0
    assert r["min_pos"].tolist() == [INF, INF] and r["max_pos"].tolist() == [-INF, -INF] and r["min_density"] == INF and r["max_density"] == -INF
    ref.check(as_struct(r), r, "empty")


def test_one_particle_and_the_terms():
    x, yy, vx, vy, rho = F(0.3), F(-0.7), F(1.1), F(2.3), F(101.5)
    r0, r1 = ref.stats(([[x, yy]], [[vx, vy]], [rho]), [(0.0, -1.0, 1.0, 0.0)])
    for r in (r0, r1):
        assert r["count"] == 1 and r["density_count"] == 1 and r["nonfinite"] == 0
        assert r["sum_pos"].tolist() == [float(x), float(yy)] and r["sum_vel"].tolist() == [float(vx), float(vy)]
        assert r["sum_speed_sq"] == float(vx) * float(vx) + float(vy) * float(vy) == r["max_speed_sq"]
        assert r["sum_angular"] == float(x) * float(vy) - float(yy) * float(vx)
        assert r["sum_density"] == float(rho) and r["sum_density_sq"] == float(rho) * float(rho)
        assert r["min_pos"].tolist() == r["max_pos"].tolist() == [x, yy] and r["min_density"] == r["max_density"] == rho
    # densities that do not belong to the positions are not read
    (r,) = ref.stats(([[x, yy]], [[vx, vy]], [rho]), density_valid=False)
    assert r["density_valid"] == 0 and r["density_count"] == 0 and r["sum_density"] == 0 and r["min_density"] == INF and r["count"] == 1


def test_nan_velocity_is_counted_and_summed_nowhere():
    pos = np.array([[0.1, 0.1], [0.2, 0.2], [0.3, 0.3], [np.nan, 0.2]], F)
    vel = np.array([[1, 0], [np.nan, 1], [0, -2], [0, 0]], F)
    rho = np.array([100, 100, np.inf, 100], F)
    r0, r1 = ref.stats((pos, vel, rho), [(0.15, 0.0, 1.0, 1.0)])
    assert (r0["count"], r0["nonfinite"], r0["density_count"]) == (2, 2, 1)  # (an infinite density: in the counts, in no density sum)
    assert r0["sum_vel"].tolist() == [1.0, -2.0] and r0["sum_speed_sq"] == 5.0 and r0["max_speed_sq"] == 4.0
    assert r0["sum_density"] == 100.0 and r0["max_pos"].tolist() == [F(0.3), F(0.3)]
    # the rectangle holds particles 1 (NaN velocity: its non-finite one) and 2; the NaN position is in no rectangle
    assert (r1["count"], r1["nonfinite"], r1["density_count"]) == (1, 1, 0)
    assert r1["sum_vel"].tolist() == [0.0, -2.0] and r1["min_density"] == INF


def test_rectangle_edges_inverted_and_overlapping():
    pos = np.array([[0.25, 0.5], [0.75, 0.5], [0.5, 0.25], [0.5, 0.75], [0.5, 0.5]], F)
    vel = np.arange(10, dtype=F).reshape(5, 2)
    rho = np.full(5, 100, F)
    rects = [(0.25, 0.25, 0.75, 0.75),   # x0 and y0 pass through particles (in), x1 and y1 too (out)
             (0.75, 0.0, 0.25, 1.0),     # inverted: empty
             (0.0, 0.0, 0.5, 1.0), (0.25, 0.4, 1.0, 0.6),  # two that overlap in particle 0
             (-INF, -INF, INF, INF)]
    r = ref.stats((pos, vel, rho), rects)
    assert [x["count"] for x in r] == [5, 3, 0, 1, 3, 5]
    assert r[1]["sum_vel"].tolist() == [0 + 4 + 8, 1 + 5 + 9]  # particles 0, 2, 4
    assert r[2]["min_pos"].tolist() == [INF, INF] and r[2]["max_speed_sq"] == 0
    assert r[3]["sum_vel"].tolist() == [0.0, 1.0] and r[4]["sum_vel"].tolist() == [0 + 2 + 8, 1 + 3 + 9]
    for k in ref.EXACT + ref.SUMS:
        assert ref.bits(r[5][k]) == ref.bits(r[0][k]), k


def test_signed_zero_extremes_and_the_bound():
    pos = np.array([[0.0, -0.0], [-0.0, 0.0], [1.0, -1.0]], F)
    (r,) = ref.stats((pos, np.zeros_like(pos), np.zeros(3, F)))
    assert ref.bits(r["min_pos"]) == ref.bits(np.array([-0.0, -1.0], F)) and ref.bits(r["max_pos"]) == ref.bits(np.array([1.0, 0.0], F))
    assert ref.bits(r["min_density"]) == ref.bits(F(0.0)) == ref.bits(r["max_density"])
    # check(): a sum off by more than n * 2^-52 * sum|t| is refused, one inside passes
    rng = np.random.default_rng(1)
    vel = rng.standard_normal((1000, 2)).astype(F)
    (r,) = ref.stats((rng.random((1000, 2), dtype=F), vel, np.ones(1000, F)))
    assert r["sum_speed_sq"] == math.fsum((vel.astype(np.float64) ** 2).sum(axis=1).tolist())
    good = as_struct(r)
    ref.check(good, r)
    near = good.copy()
    near["sum_speed_sq"] = r["sum_speed_sq"] * (1 + 500 * 2.0 ** -52)
    ref.check(near, r)
    for k, v in (("sum_speed_sq", r["sum_speed_sq"] * (1 + 1100 * 2.0 ** -52)), ("count", 999), ("max_speed_sq", np.nextafter(r["max_speed_sq"], 1e9))):
        off = good.copy()
        off[k] = v
        try:
            ref.check(off, r)
        except AssertionError:
            continue
        raise AssertionError("check() accepted a wrong %s" % k)
