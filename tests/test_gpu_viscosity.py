"""PhysicalViscosityModel on the device (k_nonpressure<PHYSICAL>, k_wcsph_accel<PHYSICAL>) against the numpy restatement of the
reference's arithmetic composed with the oracle's sub-steps (tests/viscosity_reference.py), bit for bit, through every path that reaches
the non-pressure pass: GPU tiles, the single context (step_begin / step_finish, run-ahead, the fused prediction), sphx_multi and the
headless harness.  mu = 0.01 is main.rs:96's value, 1.0016e-3 the model's default (physical.rs:14)."""
import json
import os
import subprocess

import numpy as np
import pytest
from test_tiles_cpu import run_tiles_threaded
from util import assert_bits_equal, dam_break

import yasph2d_amd as y
from tiles_reference import GpuTileBackend
from yasph2d_amd.multi import MultiSolver

pytestmark = pytest.mark.gpu

MUS = [0.01, 1.0016e-3]
HARNESS = os.path.join(os.path.dirname(os.path.abspath(y.__file__)), "sphx_harness")
DIAM = np.float32(0.01)


def physical(mu, **kw):
    return y.default_params(viscosity="physical", fluid_viscosity=mu, **kw)


def by_id(d):
    o = np.argsort(d["ids"])
    return {k: v[o] for k, v in d.items()}


def merged(outs):
    return by_id({k: np.concatenate([o[0][k] for o in outs]) for k in ("ids", "pos", "vel", "density")})


def oracle_tiles(mu, pos, boundary, steps, tiling_invariant=False, **kw):
    from viscosity_reference import PHYSICAL, ViscousOracleTileBackend

    def backend(r):
        b = ViscousOracleTileBackend(PHYSICAL, mu)
        b.o.set_tiling_invariant(tiling_invariant)
        return b

    return run_tiles_threaded(backend, pos, boundary, 2, 1, steps, **kw)[0]


def run_context(params, pos, boundary, steps, tiling_invariant=False, vel=None):
    ctx = y.SphxContext(params)
    if tiling_invariant:
        ctx.set_tiling_invariant(True)
    ctx.set_boundary(boundary)
    ctx.upload(pos, vel)
    timer = y.TimeManager()
    stats = []
    for _ in range(steps):
        vmax = ctx.step_begin(timer.simulation_step(), timer.law(DIAM))
        st = ctx.step_finish(y.duration_as_secs_f32(timer.update_simulation_step(DIAM, vmax)))
        stats.append((st["density_iterations"], st["divergence_iterations"], timer.simulation_step_ns()))
    d = by_id({k: v for k, v in ctx.download().items() if k in ("ids", "pos", "vel", "density")})
    return ctx, d, stats


@pytest.mark.parametrize("mu", MUS)
@pytest.mark.parametrize("fixed,steps", [((0, 0), 80), ((3, 2), 80)])
def test_gpu_tiles_physical_bit_exact_vs_numpy_reference(mu, fixed, steps):
    """Two strips through the impact: GPU tile contexts with the physical model against the numpy restatement on the oracle tiles."""
    pos, boundary = dam_break(1.0)
    g, _ = run_tiles_threaded(lambda r: GpuTileBackend(y.SphxContext(physical(mu))), pos, boundary, 2, 1, steps, halo=16, fixed=fixed)
    o = oracle_tiles(mu, pos, boundary, steps, halo=16, fixed=fixed)
    z = oracle_tiles(0.0, pos, boundary, steps, halo=16, fixed=fixed)
    assert not np.array_equal(merged(z)["vel"], merged(o)["vel"]), "the viscous term had no effect over these steps"
    for r in range(2):
        dg, sg, xg = g[r]
        do, so, xo = o[r]
        assert xg == xo
        for a, b in zip(sg, so):
            for k in ("density_iterations", "divergence_iterations", "dt_ns", "n_local", "n_global"):
                assert a[k] == b[k], (r, k, a[k], b[k])
        np.testing.assert_array_equal(dg["ids"], do["ids"])
        for k in ("pos", "vel", "density", "kappa"):
            assert_bits_equal(dg[k], do[k], f"rank {r} {k}")


@pytest.mark.parametrize("mu", MUS)
def test_single_context_physical_equals_the_reference_tiles_in_tiling_invariant_mode(mu):
    """The product path (sphx_step_begin / finish with the timer law, run-ahead and the fused prediction as shipped) in tiling-invariant
    mode against the reference tile run of the same mode, merged by id: bit for bit over 90 adaptive steps (free fall and impact)."""
    pos, boundary = dam_break(1.0)
    steps = 90
    ctx, d, stats = run_context(physical(mu), pos, boundary, steps, tiling_invariant=True)
    assert ctx.viscosity()[0] == "physical" and ctx.viscosity()[1] == np.float32(mu)
    ctx.close()
    o = oracle_tiles(mu, pos, boundary, steps, tiling_invariant=True, halo=16)
    ref = merged(o)
    z = merged(oracle_tiles(0.0, pos, boundary, steps, tiling_invariant=True, halo=16))
    assert not np.array_equal(z["vel"], ref["vel"]), "the viscous term had no effect over these steps"
    np.testing.assert_array_equal(d["ids"], ref["ids"])
    assert_bits_equal(d["pos"], ref["pos"], "positions")
    assert_bits_equal(d["vel"], ref["vel"], "velocities")
    for s, st in enumerate(o[0][1]):
        assert stats[s] == (st["density_iterations"], st["divergence_iterations"], st["dt_ns"]), s


def test_sphx_multi_four_tiles_physical_equals_the_single_context():
    """sphx_multi (2 x 2 tiles on one device) with the physical model: every tile context gets the model, the result is bit-equal to
    the single context in tiling-invariant mode at ~1 M particles.  The upload carries velocity jumps (1 % of the particles) so that the
    term is far from zero, and the same run with mu = 0 must differ."""
    pos, boundary = dam_break(float(np.sqrt(1.0e6 / 4050.0)))
    n, steps = len(pos), 4
    rng = np.random.default_rng(5)
    vel = np.zeros_like(pos)
    k = rng.choice(n, n // 100, replace=False)
    vel[k] = rng.normal(0.0, 0.5, (len(k), 2)).astype(np.float32)
    ctx, ref, _ = run_context(physical(0.01, fixed_iterations=(2, 2)), pos, boundary, steps, tiling_invariant=True, vel=vel)
    ctx.close()
    ctx, zero, _ = run_context(physical(0.0, fixed_iterations=(2, 2)), pos, boundary, steps, tiling_invariant=True, vel=vel)
    ctx.close()
    assert not np.array_equal(zero["vel"], ref["vel"]), "the viscous term had no effect"
    m = MultiSolver(physical(0.01, fixed_iterations=(2, 2)), devices=[0, 0, 0, 0])
    assert all(m.viscosity(k)[:2] == ("physical", np.float32(0.01)) for k in range(4))
    m.set_tiling_invariant(True)
    m.set_boundary(boundary)
    m.upload(pos, vel)
    m.steps(y.TimeManager(), steps)
    a = by_id({k: v for k, v in m.download().items() if k in ("ids", "pos", "vel")})
    m.close()
    np.testing.assert_array_equal(a["ids"], np.arange(n, dtype=np.uint32))
    assert_bits_equal(a["pos"], ref["pos"], "positions")
    assert_bits_equal(a["vel"], ref["vel"], "velocities")


def _disturbed_state(scale=1.0):
    """The device's own state after 300 XSPH steps (warm starts are dropped by the upload), with velocity jumps in a few hundred
    particles so that the viscous term is far from zero."""
    pos, boundary = dam_break(scale)
    _, d, _ = run_context(y.default_params(), pos, boundary, 300)
    vel = d["vel"].copy()
    rng = np.random.default_rng(7)
    k = rng.choice(len(vel), 300, replace=False)
    vel[k] += rng.normal(0.0, 0.5, (len(k), 2)).astype(np.float32)
    return d["pos"], vel, boundary


@pytest.mark.parametrize("mu", MUS)
def test_default_mode_one_step_after_upload_is_exact(mu):
    """Default (not tiling-invariant) mode: after an upload ids equal indices and every warm start is zero, so ordering cell mates by
    previous index or by id is the same order: one step of the single context equals one step of the reference tiles."""
    pos, vel, boundary = _disturbed_state()
    ctx, d, stats = run_context(physical(mu), pos, boundary, 1, vel=vel)
    ctx.close()
    from viscosity_reference import PHYSICAL, ViscousOracleTileBackend
    from tiles_reference import StripLayout, ThreadComm, TiledDFSPH

    t = TiledDFSPH(ViscousOracleTileBackend(PHYSICAL, mu), ThreadComm(ThreadComm.Shared(1), 0), StripLayout(1, [0, 65536]), halo=16)
    t.setup(pos, vel, None, boundary)
    st = t.step(y.TimeManager())
    ref = by_id(t.download_owned())
    assert stats[0] == (st["density_iterations"], st["divergence_iterations"], st["dt_ns"])
    assert_bits_equal(d["pos"], ref["pos"], "positions")
    assert_bits_equal(d["vel"], ref["vel"], "velocities")


SWITCHES = [({}, {}), ({}, {"list_span_limit": 16}), ({}, {"list_span_limit": y.LISTS_32BIT}), ({"SPHX_RUN_AHEAD": "0"}, {}),
            ({"SPHX_HOST_LOOP": "1"}, {}), ({"SPHX_FUSE_PREDICT": "0"}, {}), ({"SPHX_XCD_CHUNK": "0"}, {})]


def test_switch_matrix_is_bit_identical(monkeypatch):
    """Every list form nb_traverse walks (window slots, the out-of-window table, 32-bit lists) and every host/launch switch that changes
    how the non-pressure pass is reached gives the default run's bits.  From a disturbed state (velocity jumps): the runs with mu = 0
    and with XSPH must differ from the base run, so the term is exercised."""
    pos, vel, boundary = _disturbed_state(2.0)
    steps = 20
    ctx, base, bstats = run_context(physical(0.01), pos, boundary, steps, vel=vel)
    ctx.close()
    for other in (physical(0.0), y.default_params()):
        ctx, d, _ = run_context(other, pos, boundary, steps, vel=vel)
        ctx.close()
        assert not np.array_equal(d["vel"], base["vel"]), "the viscous term had no effect: the matrix would be vacuous"
    for env, fields in SWITCHES[1:]:
        with monkeypatch.context() as mp:
            for k, v in env.items():
                mp.setenv(k, v)
            p = physical(0.01)
            for k, v in fields.items():
                setattr(p, k, v)
            ctx, d, stats = run_context(p, pos, boundary, steps, vel=vel)
            ctx.close()
        assert stats == bstats, (env, fields)
        assert_bits_equal(d["pos"], base["pos"], f"positions {env} {fields}")
        assert_bits_equal(d["vel"], base["vel"], f"velocities {env} {fields}")


def test_physical_differs_from_xsph_after_one_step():
    """Negative control: a launch site that ignored the model would pass every equality above with XSPH on both sides."""
    pos, vel, boundary = _disturbed_state()
    _, a, _ = run_context(y.default_params(), pos, boundary, 1, vel=vel)
    _, b, _ = run_context(physical(0.01), pos, boundary, 1, vel=vel)
    assert not np.array_equal(a["vel"], b["vel"])
    ca, cb = y.SphxContext(y.default_params()), y.SphxContext(physical(0.01))
    assert ca.viscosity()[0] == "xsph" and cb.viscosity()[0] == "physical"
    from viscosity_reference import Constants

    assert cb.viscosity()[2] == Constants().vis_nlap  # Viscosity::new's normalizer_laplacian, the host's and the restatement's
    ca.close()
    cb.close()


def test_wcsph_physical_per_step_bit_exact_vs_numpy_reference():
    """k_wcsph_accel<physical> against the numpy restatement of update_accellerations (viscosity_reference.wcsph_*), chained over 30
    WCSPH steps from a fresh context (the accelerations are zero) with velocity jumps in the upload.  Per step: v_1/2 and the positions
    from the previous step's numpy accelerations must equal the device's positions (by id); with the device's own lists, Poly6
    densities and boundary, the numpy vmax, the dt a second timer derives from it and the final velocities must equal the device's,
    bit for bit.  Guard: the physical term changes the accelerations (mu = 0 gives others)."""
    from test_viscosity_host import wcsph_disturbed
    from viscosity_reference import PHYSICAL, Constants, wcsph_accel, wcsph_finish, wcsph_leapfrog1

    mu = np.float32(0.01)
    K = Constants()
    pos, vel, boundary = wcsph_disturbed()
    ctx = y.SphxContext(physical(0.01))
    ctx.set_boundary(boundary)
    ctx.upload(pos, vel)
    timer, twin = y.TimeManager(cfl_factor=0.2), y.TimeManager(cfl_factor=0.2)
    P, V, ids = pos.copy(), vel.copy(), np.arange(len(pos), dtype=np.uint32)
    A = np.zeros_like(pos)
    moved = 0
    for s in range(30):
        dt = np.float32(timer.simulation_step())
        Pn, Vh = wcsph_leapfrog1(P, V, A, dt)
        vmax = ctx.wcsph_step_begin(dt)
        dt_ns = timer.update_simulation_step(DIAM, vmax)
        ctx.wcsph_step_finish(y.duration_as_secs_f32(dt_ns))
        d = ctx.download()
        inv = np.empty(len(ids), np.int64)
        inv[ids] = np.arange(len(ids))
        perm = inv[d["ids"]]  # previous slot of each particle in the device's new order
        assert_bits_equal(d["pos"], Pn[perm], f"step {s} positions")
        nb = ctx.download_neighbors()
        bnd, _ = ctx.download_boundary()
        acc, vmax_np, dt_np, vel_np = wcsph_finish(PHYSICAL, mu, K, d["pos"], Vh[perm], d["density"], bnd, nb, dt, twin, DIAM)
        assert np.float32(vmax) == vmax_np, (s, vmax, vmax_np)
        assert dt_np == dt_ns, s
        assert_bits_equal(d["vel"], vel_np, f"step {s} velocities")
        if s == 0:
            a0 = wcsph_accel(PHYSICAL, np.float32(0.0), K, d["pos"], Vh[perm], d["density"], bnd, nb, dt)
            moved = int((a0 != acc).any(axis=1).sum())
        P, V, A, ids = d["pos"], d["vel"], acc, d["ids"]
    ctx.close()
    assert moved > 100, "the viscous term changed too few accelerations to exercise the walk"


def test_wcsph_physical_ignores_the_list_form():
    """32-bit lists give the bits of the default lists for the physical WCSPH step (from the same disturbed state)."""
    from test_viscosity_host import wcsph_disturbed

    pos, vel, boundary = wcsph_disturbed()
    out = []
    for limit in (0, y.LISTS_32BIT):
        p = physical(0.01)
        p.list_span_limit = limit
        ctx = y.SphxContext(p)
        ctx.set_boundary(boundary)
        ctx.upload(pos, vel)
        timer = y.TimeManager(cfl_factor=0.2)
        for _ in range(30):
            vmax = ctx.wcsph_step_begin(timer.simulation_step())
            ctx.wcsph_step_finish(y.duration_as_secs_f32(timer.update_simulation_step(DIAM, vmax)))
        out.append((by_id({k: v for k, v in ctx.download().items() if k in ("ids", "pos", "vel")}), timer.simulation_step_ns()))
        ctx.close()
    (a, ta), (b, tb) = out
    assert ta == tb
    assert_bits_equal(a["pos"], b["pos"], "positions")
    assert_bits_equal(a["vel"], b["vel"], "velocities")


def test_harness_physical_matches_the_python_driver():
    from test_gpu_harness import fnv1a

    steps = 120
    xs = subprocess.run([HARNESS, "--viscosity", "xsph", "--scale", "1", "--steps", str(steps), "--warmup", "0"], capture_output=True, text=True,
                        timeout=600)
    assert xs.returncode == 0, xs.stderr
    out = subprocess.run([HARNESS, "--viscosity", "physical:0.01", "--scale", "1", "--steps", str(steps), "--warmup", "0"], capture_output=True,
                         text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    res = json.loads(out.stdout.strip().splitlines()[-1])
    assert res["viscosity"] == "physical" and np.float32(res["fluid_viscosity"]) == np.float32(0.01)
    w = y.FluidParticleWorld()
    w.reset_fluid(1.0)
    ctx = y.SphxContext(physical(0.01))
    ctx.set_boundary(w.boundary_particles)
    ctx.upload(w.positions)
    timer = y.TimeManager()
    for _ in range(steps):
        timer.on_step_started()
        vmax = ctx.step_begin(timer.simulation_step(), timer.law(DIAM))
        ctx.step_finish(y.duration_as_secs_f32(timer.update_simulation_step(DIAM, vmax)))
    d = ctx.download()
    rec = np.zeros((len(d["ids"]), 4), np.float32)
    rec[d["ids"], :2] = d["pos"]
    rec[d["ids"], 2:] = d["vel"]
    assert res["timer_step_ns"] == timer.simulation_step_ns()
    assert int(res["state_fnv1a"], 16) == fnv1a(rec.tobytes())
    assert json.loads(xs.stdout.strip().splitlines()[-1])["state_fnv1a"] != res["state_fnv1a"], "the model made no difference"


def test_harness_rejects_a_malformed_viscosity():
    for arg in ("physical:abc", "physical:", "physical:0.01x", "xsph:0.1", "sph"):
        out = subprocess.run([HARNESS, "--viscosity", arg, "--steps", "1"], capture_output=True, text=True, timeout=60)
        assert out.returncode == 2, (arg, out.stderr)
