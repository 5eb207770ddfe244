"""Field sampling without a GPU: the C ABI exports the two calls and checks its context argument; the float32 restatement of the
sampling contract (tests/sample_reference.py), which the GPU tests compare the device with bit for bit, is itself checked against
hand-made cases, a float64 brute force and the oracle's neighbour lists and densities."""
import ctypes as C

import numpy as np
import pytest

import sample_reference as sr
import yasph2d_amd as y
from util import dam_break
from yasph2d_amd import _lib

F = np.float32


def test_sampling_symbols_exported_and_null_context_rejected(sphx_lib):
    assert hasattr(sphx_lib, "sphx_sample_points") and hasattr(sphx_lib, "sphx_sample_grid")
    for name in ("sphx_sample_points", "sphx_sample_grid"):
        assert name in _lib.SIGNATURES
    d = np.zeros(4, np.float32)
    out = _lib.SphxSampleOut(density=d.ctypes.data)
    xy = np.zeros((4, 2), np.float32)
    assert sphx_lib.sphx_sample_points(None, xy.ctypes.data_as(C.c_void_p), 4, 0, 0, C.byref(out)) == _lib.ERR_INVALID_ARGUMENT
    assert sphx_lib.sphx_sample_grid(None, 0.0, 0.0, 0.1, 0.1, 2, 2, 0, 0, C.byref(out)) == _lib.ERR_INVALID_ARGUMENT
    assert y.SAMPLE_FIELDS == sr.FIELDS


def _consts():
    return sr.Constants(y.default_params())


def _state(pos, vel, rho, bnd=None):
    return dict(pos=np.asarray(pos, F).reshape(-1, 2), vel=np.asarray(vel, F).reshape(-1, 2), density=np.asarray(rho, F),
                boundary=np.zeros((0, 2), F) if bnd is None else np.asarray(bnd, F).reshape(-1, 2))


@pytest.mark.parametrize("kind", [sr.KERNEL_WENDLAND, sr.KERNEL_POLY6, sr.KERNEL_SPIKY])
def test_single_particle(kind):
    K = _consts()
    p = np.array([[0.5, 0.5]], F)
    v = np.array([[0.37, -1.9]], F)
    st = _state(p, v, [F(101.25)])
    q = (p + np.array([[0.0071, -0.0042]], F)).astype(F)
    out = sr.sample32(K, st, q, kind)
    d = (p - q).astype(F)
    d2 = F(F(d[0, 0] * d[0, 0]) + F(d[0, 1] * d[0, 1]))
    w = sr.w32(K, kind, np.array([d2]))[0]
    assert w > 0 and out["density"][0] == F(w * K.mass) and out["count"][0] == 1
    a = F(F(K.mass / F(101.25)) * w)
    assert out["fraction"][0] == a
    # (a v) / a: within one ulp of v
    np.testing.assert_array_max_ulp(out["velocity"][0], v[0], maxulp=1)
    # far away: nothing, velocity (0, 0)
    far = sr.sample32(K, st, np.array([[0.5 + 3 * K.h, 0.5]], F), kind)
    assert far["density"][0] == 0 and far["fraction"][0] == 0 and far["count"][0] == 0 and not far["velocity"].any()


def test_two_symmetric_particles_and_the_radius():
    K = _consts()
    c = np.array([0.25, 0.75], F)
    off = np.array([2.0 ** -8, 0.0], F)  # (exact: c - off and c + off are symmetric in fp32)
    p = np.stack([c - off, c + off]).astype(F)
    v = np.array([[1.0, 2.0], [-1.0, 2.0]], F)
    st = _state(p, v, [100.0, 100.0])
    out = sr.sample32(K, st, c[None], sr.KERNEL_WENDLAND)
    w = sr.w32(K, sr.KERNEL_WENDLAND, np.array([F(off[0] * off[0])]))[0]
    assert out["count"][0] == 2 and out["density"][0] == F(F(w * K.mass) + F(w * K.mass))
    assert out["velocity"][0, 0] == 0 and out["velocity"][0, 1] == F(2.0)
    # the farthest point at d2 <= radius_sq (fp32) from a particle: accepted, W ~ 0 there; one ulp further: not
    def d2_of(qx):
        d = F(p[0, 0] - qx)
        return F(d * d)

    qx = F(p[0, 0] - K.h)
    while d2_of(qx) > K.radius_sq:
        qx = np.nextafter(qx, F(1))
    while d2_of(np.nextafter(qx, F(-1))) <= K.radius_sq:
        qx = np.nextafter(qx, F(-1))  # (the farthest point still at d2 <= h*h)
    q = np.array([[qx, p[0, 1]]], F)
    for kind in (sr.KERNEL_WENDLAND, sr.KERNEL_POLY6, sr.KERNEL_SPIKY):
        o = sr.sample32(K, _state(p[:1], v[:1], [100.0]), q, kind)
        assert o["count"][0] == 1 and (kind == sr.KERNEL_POLY6 or o["density"][0] < F(1e-12) * sr.w32(K, kind, np.zeros(1, F))[0])
    q2 = np.array([[np.nextafter(q[0, 0], F(-1)), q[0, 1]]], F)
    assert sr.sample32(K, _state(p[:1], v[:1], [100.0]), q2, sr.KERNEL_WENDLAND)["count"][0] == 0
    # a point exactly on a particle: d2 = 0 is accepted (not "self"), W(0)
    o = sr.sample32(K, _state(p[:1], v[:1], [100.0]), p[:1], sr.KERNEL_WENDLAND)
    assert o["count"][0] == 1 and o["density"][0] == F(sr.w32(K, sr.KERNEL_WENDLAND, np.zeros(1, F))[0] * K.mass)


def _oracle_state(steps, wcsph=False):
    from oracle.oracle import Oracle

    pos, boundary = dam_break(1.0)
    o = Oracle()
    if wcsph:
        t = y.TimeManager(cfl_factor=0.2)
        o.timer_adaptive(t.timestep_max_ns, t.timestep_min_ns, 0.2)
    o.set_boundary(boundary)
    o.set_particles(pos)
    for _ in range(steps):
        o.wcsph_step() if wcsph else o.dfsph_step()
    st = dict(pos=o.positions(), vel=o.velocities(), density=o.densities(), boundary=o.boundary())
    return o, st


def _probe_points(st, K, seed):
    """particle positions, a jittered set around them, a lattice over the scene, points next to and inside the walls, far away, NaN/inf"""
    rng = np.random.default_rng(seed)
    pos, bnd = st["pos"], st["boundary"]
    pts = [pos[rng.choice(len(pos), 300, replace=False)],
           (pos[rng.choice(len(pos), 300, replace=False)] + rng.normal(0, float(K.h), (300, 2))).astype(F),
           sr.lattice_points(-0.05, -0.05, 0.037, 0.041, 60, 70),
           (bnd[rng.choice(len(bnd), 100, replace=False)] + rng.normal(0, float(K.h) / 3, (100, 2))).astype(F),
           np.array([[1e6, 1e6], [-1e30, 0.5], [np.nan, 0.5], [0.5, np.nan], [np.inf, 0.5], [-np.inf, -np.inf], [-200, -200]], F)]
    return np.concatenate(pts).astype(F)


@pytest.mark.parametrize("steps, wcsph", [(1, False), (60, False), (30, True)])
def test_restatement_within_float64_bound_on_oracle_states(steps, wcsph):
    o, st = _oracle_state(steps, wcsph)
    K = _consts()
    params = y.default_params()
    pts = _probe_points(st, K, steps)
    for kind in (sr.KERNEL_WENDLAND, sr.KERNEL_POLY6, sr.KERNEL_SPIKY):
        dev = sr.sample32(K, st, pts, kind)
        ref, mag, terms = sr.sample64(params, st, pts, kind)
        r = sr.assert_within_bound(dev, ref, mag, terms, "steps %d kind %d" % (steps, kind))
        assert max(r.values()) < 0.5, r
        # (non-finite and far points: zeros, count 0)
        tail = slice(len(pts) - 7, len(pts))
        assert not dev["density"][tail].any() and not dev["count"][tail].any() and not dev["velocity"][tail].any()
    # guard: a slip of the contract (e.g. the boundary left out of the density) is far beyond the bound
    bad = sr.sample32(K, dict(st, boundary=np.zeros((0, 2), F)), pts, sr.KERNEL_WENDLAND)
    ref, mag, terms = sr.sample64(params, st, pts, sr.KERNEL_WENDLAND)
    assert sr.bound_ratios(bad, ref, mag, terms)["density"] > 100


@pytest.mark.parametrize("steps, wcsph", [(1, False), (60, False), (30, True)])
def test_restatement_at_particles_matches_the_oracle_lists_and_densities(steps, wcsph):
    o, st = _oracle_state(steps, wcsph)
    K = _consts()
    counts, _, _ = o.neighbors()
    assert counts[:, 0].max() < 64, "capped lists: count_dynamic + 1 would not hold"
    kind = sr.KERNEL_POLY6 if wcsph else sr.KERNEL_WENDLAND  # the solver's density kernel (wscsph.rs:32, dfsph.rs)
    out = sr.sample32(K, st, st["pos"], kind)
    p = st["pos"].astype(np.float64)
    # (no pair closer than 1e-5: the build's d2 > 1e-10 exclusion then only drops the particle itself)
    qi, j, d2 = sr._pairs_within(float(K.h), st["pos"], st["pos"])
    assert d2[qi != j].min() > 1e-10
    np.testing.assert_array_equal(out["count"], counts[:, 0].astype(np.uint32) + 1)
    ref, mag, terms = sr.sample64(y.default_params(), st, st["pos"], kind)
    clamped = np.maximum(out["density"], K.rho0)
    err = np.abs(clamped.astype(np.float64) - o.densities().astype(np.float64))
    bound = sr.C * (terms["density"] + sr.K["density"]) * sr.U * mag["density"]
    assert (err <= bound).all(), float((err / bound).max())
    assert (o.densities() >= K.rho0).all() and np.isfinite(p).all()


def test_gauge_rule():
    ny, ys = sr.gauge_column(0.0, 2.5, 0.0025)
    assert ny == 1001 and ys[0] == 0 and ys[-1] == F(F(1000) * F(0.0025))
    f = np.zeros(ny, F)
    f[:200] = 1.0
    f[200] = 0.75
    f[201] = 0.25
    e = sr.elevation(ys, f)
    assert e == pytest.approx(float(ys[200]) + 0.5 * (float(ys[201]) - float(ys[200])), rel=1e-12)
    assert np.isnan(sr.elevation(ys, np.zeros(ny, F)))
    assert sr.elevation(ys, np.ones(ny, F)) == float(ys[-1])
    # the library's own helper applies the same rule
    assert y._elevation(ys, f) == e and np.isnan(y._elevation(ys, np.zeros(ny, F)))
