"""The viscosity model choice (sphx_params.viscosity_model / .fluid_viscosity) without a GPU: defaults, validation in sphx_create
before any device is queried, the Python keywords, and the numpy restatement the GPU tests compare against (tests/
viscosity_reference.py), proven faithful in its XSPH form against the oracle bit for bit."""
import ctypes as C

import numpy as np
import pytest
from test_tiles_cpu import run_tiles_threaded
from util import dam_break

import yasph2d_amd as y
from yasph2d_amd import _lib
from yasph2d_amd.multi import MultiSolver


def test_default_params_keep_xsph_and_fill_the_water_viscosity(sphx_lib):
    p = _lib.SphxParams()
    assert sphx_lib.sphx_default_params(2.0, 10000.0, 100.0, C.byref(p)) == _lib.OK
    assert p.viscosity_model == _lib.VISCOSITY_XSPH == y.VISCOSITY_XSPH == 0
    assert np.float32(p.fluid_viscosity) == np.float32(1.0016) / np.float32(1000.0)  # physical.rs:14, f32 division
    assert list(p.reserved) == [0]
    assert C.sizeof(_lib.SphxParams) == 80
    assert _lib.SphxParams.viscosity_model.offset == 68 and _lib.SphxParams.fluid_viscosity.offset == 72  # the former reserved[0..1]


@pytest.mark.parametrize("field,value,text", [("viscosity_model", 2, "viscosity_model"), ("viscosity_model", 0xFFFFFFFF, "viscosity_model"),
                                              ("fluid_viscosity", float("nan"), "fluid_viscosity"),
                                              ("fluid_viscosity", float("inf"), "fluid_viscosity"),
                                              ("fluid_viscosity", float("-inf"), "fluid_viscosity")])
def test_create_rejects_an_unknown_model_or_a_non_finite_viscosity(sphx_lib, field, value, text):
    """Checked with the other parameter checks, before the device is queried: the same answer with or without a GPU."""
    p = y.default_params()
    setattr(p, field, value)
    h = C.c_void_p()
    assert sphx_lib.sphx_create(C.byref(p), C.byref(h)) == _lib.ERR_INVALID_ARGUMENT
    assert not h.value
    assert text in sphx_lib.sphx_last_error(None).decode()
    with pytest.raises(y.SphxError) as e:
        y.SphxContext(p)
    assert e.value.code == _lib.ERR_INVALID_ARGUMENT
    with pytest.raises(y.SphxError) as e:
        MultiSolver(p, devices=[0, 0])
    assert e.value.code == _lib.ERR_INVALID_ARGUMENT


def test_negative_viscosity_passes_validation(sphx_lib):
    """PhysicalViscosityModel takes any f32: a negative mu is not a parameter error (without a device the create fails later, at the
    device query)."""
    import torch

    p = y.default_params(viscosity="physical", fluid_viscosity=-0.5)
    h = C.c_void_p()
    rc = sphx_lib.sphx_create(C.byref(p), C.byref(h))
    if torch.cuda.is_available():
        assert rc == _lib.OK
        sphx_lib.sphx_destroy(h)
    else:
        assert rc == _lib.ERR_NO_DEVICE


def test_python_keywords():
    p = y.default_params(viscosity="physical", fluid_viscosity=0.01)
    assert p.viscosity_model == y.VISCOSITY_PHYSICAL == 1 and np.float32(p.fluid_viscosity) == np.float32(0.01)
    q = y.default_params(viscosity="physical")
    assert np.float32(q.fluid_viscosity) == np.float32(1.0016) / np.float32(1000.0)
    r = y.default_params(fixed_iterations=(3, 2))
    assert r.viscosity_model == y.VISCOSITY_XSPH and (r.fixed_density_iterations, r.fixed_divergence_iterations) == (3, 2)
    with pytest.raises(ValueError):
        y.default_params(viscosity="sph")
    assert _lib.SIGNATURES["sphx_get_viscosity"][0] is C.c_int
    assert _lib.lib().sphx_get_viscosity(None, None, None, None) == _lib.ERR_INVALID_ARGUMENT


def test_laplacian_normalizer_follows_the_reference_expression():
    """360 / (29 * (PI as f32) * h.powi(5)) in f32, left to right (viscosity.rs:24), for the app's h = 0.02."""
    from viscosity_reference import Constants, rs_powi

    K = Constants()
    h = np.float32(0.02)
    assert K.h == h
    p5 = np.float32(np.float32(np.float32(h * h) * np.float32(h * h)) * h)  # __powisf2(h, 5): r = h; a = h^2; a = h^4; r *= a
    assert rs_powi(h, 5) == p5
    assert K.vis_nlap == np.float32(360.0) / np.float32(np.float32(np.float32(29.0) * np.float32(np.pi)) * p5)


def test_numpy_xsph_restatement_reproduces_the_oracle_tiles_bit_for_bit():
    """ViscousOracleTileBackend in XSPH mode replaces the oracle's non-pressure pass and prediction by the numpy restatement; over 80
    adaptive steps of the 2-strip dam break (free fall, impact, splash) it must agree with OracleTileBackend bit for bit.  This proves the
    composition (state written back, re-grid of unmoved positions) and the list-order masked summation before the physical form — the
    same code with another scalar — is trusted.  Guard: with epsilon = 0 the run differs, so the term is not zero over these steps."""
    from tile_oracle_backend import OracleTileBackend
    from viscosity_reference import XSPH, ViscousOracleTileBackend

    pos, boundary = dam_break(1.0)
    steps = 80
    eps = y.default_params().xsph_epsilon
    a, _ = run_tiles_threaded(lambda r: OracleTileBackend(), pos, boundary, 2, 1, steps)
    b, _ = run_tiles_threaded(lambda r: ViscousOracleTileBackend(XSPH, eps), pos, boundary, 2, 1, steps)
    z, _ = run_tiles_threaded(lambda r: ViscousOracleTileBackend(XSPH, 0.0), pos, boundary, 2, 1, steps)
    for r in range(2):
        da, sa, xa = a[r]
        db, sb, xb = b[r]
        assert xa == xb
        for p, q in zip(sa, sb):
            for k in ("density_iterations", "divergence_iterations", "dt_ns", "n_local", "n_global"):
                assert p[k] == q[k], (r, k)
        np.testing.assert_array_equal(da["ids"], db["ids"])
        for k in ("pos", "vel", "density", "kappa", "stiffness"):
            assert np.array_equal(da[k].view(np.uint32), db[k].view(np.uint32)), (r, k)
    assert any(len(z[r][0]["vel"]) != len(b[r][0]["vel"]) or not np.array_equal(z[r][0]["vel"], b[r][0]["vel"]) for r in range(2)), \
        "the XSPH term had no effect: the comparison would not see a wrong summation"


def wcsph_disturbed(scale=1.0, seed=3):
    """The reference scene with velocity jumps in 300 particles: the viscous term is far from zero from the first step on."""
    pos, boundary = dam_break(scale)
    rng = np.random.default_rng(seed)
    vel = np.zeros_like(pos)
    k = rng.choice(len(pos), 300, replace=False)
    vel[k] = rng.normal(0.0, 0.5, (len(k), 2)).astype(np.float32)
    return pos, vel, boundary


def numpy_wcsph_run(model, coef, pos, vel, boundary, steps):
    """WCSPH steps with update_accellerations in numpy (viscosity_reference.wcsph_*); a second oracle only re-grids and computes the
    Poly6 densities (update_neighborhood_datastructure + update_densities, wscsph.rs:152-153) -> [(vmax, dt_ns)], positions, velocities."""
    from oracle.oracle import KERNEL_POLY6, Oracle
    from viscosity_reference import Constants, wcsph_finish, wcsph_leapfrog1

    K = Constants()
    prov = Oracle()
    prov.set_boundary(boundary)
    timer = y.TimeManager(cfl_factor=0.2)
    acc = np.zeros_like(pos)  # accellerations.resize(n, zero), wscsph.rs:129
    out = []
    for _ in range(steps):
        dt = np.float32(timer.simulation_step())
        pos, vel = wcsph_leapfrog1(pos, vel, acc, dt)
        prov.set_particles(pos, vel)
        prov.update_neighborhood()
        prov.update_densities(KERNEL_POLY6)
        pos, vel = prov.positions(), prov.velocities()
        acc, vmax, dt_ns, vel = wcsph_finish(model, coef, K, pos, vel, prov.densities(), prov.boundary(), prov.neighbors(), dt, timer,
                                             np.float32(0.01))
        out.append((vmax, dt_ns))
    return out, pos, vel


def test_numpy_wcsph_restatement_reproduces_orc_wcsph_step_bit_for_bit():
    """The WCSPH restatement in XSPH mode against the oracle's WCSPHSolver::simulation_step (orc_wcsph_step) over 20 steps from a
    state with velocity jumps: vmax, dt, positions and velocities bit for bit.  Guard: with epsilon = 0 the velocities differ."""
    from oracle.oracle import Oracle
    from viscosity_reference import XSPH

    pos, vel, boundary = wcsph_disturbed()
    steps = 20
    o = Oracle()
    t = y.TimeManager(cfl_factor=0.2)
    o.timer_adaptive(t.timestep_max_ns, t.timestep_min_ns, 0.2)
    o.set_boundary(boundary)
    o.set_particles(pos, vel)
    ref = []
    for _ in range(steps):
        st = o.wcsph_step()
        ref.append((np.float32(st["vmax"]), o.timer_step_ns()))
    eps = y.default_params().xsph_epsilon
    got, p, v = numpy_wcsph_run(XSPH, eps, pos, vel, boundary, steps)
    assert got == ref
    assert np.array_equal(p.view(np.uint32), o.positions().view(np.uint32))
    assert np.array_equal(v.view(np.uint32), o.velocities().view(np.uint32))
    _, _, v0 = numpy_wcsph_run(XSPH, 0.0, pos, vel, boundary, steps)
    assert not np.array_equal(v0, v), "the XSPH term had no effect"


def test_physical_restatement_differs_from_xsph_and_damps():
    """Sanity of the physical form on the oracle's own state: a velocity jump between neighbours is reduced, not amplified."""
    from oracle.oracle import Oracle
    from viscosity_reference import PHYSICAL, XSPH, Constants, nonpressure_accel

    pos, boundary = dam_break(1.0)
    o = Oracle()
    o.set_boundary(boundary)
    o.set_particles(pos)
    o.update_neighborhood()
    o.update_densities()
    p = o.positions()
    vel = np.zeros_like(p)
    vel[: len(p) // 2, 0] = np.float32(1.0)
    nb = o.neighbors()
    K = Constants()
    dt = np.float32(0.001)
    ap = nonpressure_accel(PHYSICAL, np.float32(0.01), K, p, vel, o.densities(), nb, dt)
    ax = nonpressure_accel(XSPH, np.float32(0.05), K, p, vel, o.densities(), nb, dt)
    assert not np.array_equal(ap, ax)
    moving = vel[:, 0] > 0
    assert (ap[moving, 0] <= 0).all() and (ap[~moving, 0] >= 0).all()
    assert (ap[:, 0] != 0).sum() > 0
