"""The device's DFSPH against the float64 restatement of the Rust solver (tests/dfsph_reference64.py).

(1) Sub-steps: GpuTileBackend, one tile over the whole domain, lock-step through the plan of TiledDFSPH.step with a download after
every sub-step, compared within the round-off bound of tests/dfsph_lockstep.py (C = 2, per-output allowances K there) — plain and
fused forms (sphx_sub_predict_iteration, sphx_sub_regrid_div / _warm), the scenes of test_dfsph_reference64 and the A/B switches
and list formats that only large contexts take by default, forced at small N.  Downloading between sub-steps changes nothing.
(2) Whole steps of the product path (SphxContext step_begin / step_finish) at fixed (1, 1) and (3, 2) iterations from a disturbed
state with live warm starts, restated in float64 from the state before the step; adaptive iteration counts against the float64
stop tests.  (3) sphx_update_densities for the three kernels.  (4) One 16 M-particle context, sampled.  (5) Every mutant of the
restatement is rejected on the device's data."""
import numpy as np
import pytest
import test_dfsph_reference64 as cpu
from dfsph_lockstep import (MUTANTS, Bounds, BoundaryScaled, NoWarmStartDamping, check_trace, context_state, make_plan,
                            membership_of_trace, mutant, restate_step, restatement, run_and_check, run_plan, single_tile, step_deviation,
                            _combined)
from dfsph_reference64 import KERNEL_POLY6, KERNEL_SPIKY, KERNEL_WENDLAND
from util import dam_break

import yasph2d_amd as y
from tiles_reference import GpuTileBackend

pytestmark = pytest.mark.gpu

H = cpu.H
# Whole steps: max |dev - ref| / max |ref| per output.  Measured: <= 6e-5 (positions, relative to the step's largest displacement;
# alpha 2e-5, the rest <= 7e-6); the weakest mutant that applies at whole-step level exceeds 0.14 (the warm start without its
# damping at (3, 2); at (1, 1): the divergence walk on pre-advect positions, 0.97).  1e-3 sits 16x above the one and 140x below
# the other.  (The boundary terms scaled by 1.001 change a whole step by less than its round-off: that mutant is rejected by the
# sub-step comparison only.)
STEP_TOL = 1e-3


def device_trace(make, steps, fixed, fuse=False, env=None, monkeypatch=None, span=None, record=True):
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    p = y.default_params()
    if span is not None:
        p.list_span_limit = span
    b = GpuTileBackend(y.SphxContext(p), own_stream=False)
    pos, vel, boundary = make()
    single_tile(b, pos, vel, boundary)
    out = run_plan(b, make_plan(steps, fixed, fuse_predict=fuse, regrid="fused" if fuse else "plain"), record=record)
    b.ctx.close()
    return out


def check_device(trace, name):
    bounds = check_trace(trace, restatement(), Bounds(), name)
    print(f"\n{name}: worst ratios\n{bounds.report()}")
    bounds.assert_within()
    membership_of_trace(trace, H)
    return bounds


GPU_SCENES = ["dam_break", "random", "dense_cluster", "spray", "boundary_only", "lattice_at_h", "n1", "n63", "n64", "n65", "n255",
              "n256", "n257", "n1023", "n1024", "n1025", "n4097"]


@pytest.mark.parametrize("fuse", [False, True], ids=["plain", "fused"])
@pytest.mark.parametrize("name", GPU_SCENES)
def test_device_substeps_match_float64_restatement(name, fuse):
    make, steps, fixed = cpu.SCENES[name]
    check_device(device_trace(make, steps, fixed, fuse), f"{name} {'fused' if fuse else 'plain'}")


SWITCHES = [({"SPHX_STREAM_LISTS": "1", "SPHX_NT_COLD_STORES": "1"}, None), ({"SPHX_LAZY_TABLE": "0"}, None), ({"SPHX_QCLAMP": "1"}, None),
            ({"SPHX_FUSE_PREDICT": "0", "SPHX_FUSE_DIV": "0", "SPHX_FUSE_WARM": "0"}, None), ({}, y.LISTS_32BIT), ({}, 60), ({}, 130)]


@pytest.mark.parametrize("env,span", SWITCHES, ids=lambda v: (",".join(f"{k}={x}" for k, x in v.items()) or "default") if isinstance(v, dict)
                         else f"span{v}")
@pytest.mark.parametrize("name", ["dam_break", "dense_cluster", "spray"])
def test_device_substeps_under_switches(monkeypatch, name, env, span):
    make, steps, fixed = cpu.SCENES[name]
    check_device(device_trace(make, steps, fixed, True, env, monkeypatch, span), f"{name} {env} {span}")
    check_device(device_trace(make, steps, fixed, False, env, monkeypatch, span), f"{name} {env} {span} plain")


def test_downloads_between_substeps_change_nothing():
    make, steps, fixed = cpu.SCENES["dam_break"]
    for fuse in (False, True):
        a = device_trace(make, 3, fixed, fuse)[-1][3]
        b = device_trace(make, 3, fixed, fuse, record=False)
        for k in ("pos", "vel", "density", "alpha", "kappa", "stiffness", "ids", "counts", "lists"):
            assert np.array_equal(np.asarray(a[k]).view(np.uint8), np.asarray(b[k]).view(np.uint8)), (fuse, k)


@pytest.mark.parametrize("cls", MUTANTS, ids=lambda c: c.__name__)
def test_mutant_is_rejected_on_device_data(cls):
    ratio = 0.0
    for name in ("dam_break", "spray"):
        make, steps, fixed = cpu.SCENES[name]
        for fuse in (False, True):
            ratio = max(ratio, check_trace(device_trace(make, steps, fixed, fuse), mutant(cls), Bounds(), name).max_ratio())
    print(f"\n{cls.__name__}: {ratio:.3g} x the bound")
    assert ratio > 1.0, f"mutant '{cls.__doc__}' passes the comparison on device data (ratio {ratio:.3g})"


# ------------------------------------------------------------------------------------------------------------------ whole steps
def disturbed_context(fixed, warmup=3, env=None, monkeypatch=None):
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    pos, vel, boundary = cpu.dam_break_disturbed()
    ctx = y.SphxContext(y.default_params(fixed_iterations=fixed))
    ctx.set_boundary(boundary)
    ctx.upload(pos, vel)
    timer = y.TimeManager()
    for _ in range(warmup):
        device_step(ctx, timer)
    return ctx, timer


def device_step(ctx, timer):
    dt_prev = timer.simulation_step()
    vmax = ctx.step_begin(dt_prev)
    dt = y.duration_as_secs_f32(timer.update_simulation_step(np.float32(0.01), vmax))
    st = ctx.step_finish(dt)
    st["dt_prev"], st["dt"], st["vmax"] = float(np.float32(dt_prev)), float(np.float32(dt)), float(np.float32(vmax))
    return st


def whole_steps(ctx, timer, fixed, refs, steps=3):
    worst = {}
    for _ in range(steps):
        pre = context_state(ctx)
        st = device_step(ctx, timer)
        post = context_state(ctx)
        assert (st["density_iterations"], st["divergence_iterations"]) == fixed
        warm = (bool(st["warmstart_density"]), bool(st["warmstart_divergence"]))
        assert warm == (fixed[0] > 1, fixed[1] > 1)  # dfsph.rs:199,354: the previous step needed more than one iteration
        for name, r in refs.items():
            d = step_deviation(restate_step(r, pre, post, st["dt_prev"], st["dt"], fixed, warm), post, st)
            worst[name] = max(worst.get(name, 0.0), max(d.values()))
            if name == "faithful":
                assert max(d.values()) <= STEP_TOL, d
    return worst


@pytest.mark.parametrize("fixed", [(1, 1), (3, 2)])
@pytest.mark.parametrize("env", [{}, {"SPHX_STREAM_LISTS": "1", "SPHX_NT_COLD_STORES": "1"}, {"SPHX_FUSE_PREDICT": "0", "SPHX_FUSE_DIV": "0",
                                                                                                "SPHX_FUSE_WARM": "0"}],
                         ids=["default", "stream_nt", "unfused"])
def test_whole_steps_match_float64_restatement(monkeypatch, fixed, env):
    ctx, timer = disturbed_context(fixed, env=env, monkeypatch=monkeypatch)
    refs = {"faithful": restatement()}
    skip = (BoundaryScaled,) + ((NoWarmStartDamping,) if fixed == (1, 1) else ())
    refs.update({c.__name__: mutant(c) for c in MUTANTS if c not in skip})
    worst = whole_steps(ctx, timer, fixed, refs)
    print(f"\nwhole steps {fixed}: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    for name, v in worst.items():
        if name != "faithful":
            assert v > 10 * STEP_TOL, (name, v)


def test_adaptive_iteration_counts_follow_the_float64_stop_tests():
    """Adaptive loops: each step's iteration counts are where the float64 residuals first pass the stop tests (dfsph.rs:226,381),
    except where a float64 residual lies within the whole-step bound of its threshold (such steps must be rare)."""
    from dfsph_reference64 import MAX_AVG_DENSITY_ERROR, MAX_DIVERGENCE_ERROR

    ctx, timer = disturbed_context((0, 0), warmup=1)  # the first step also runs the warm-up block (dfsph.rs:419-428)
    ref = restatement()
    close, steps, iterating = 0, 40, 0
    for _ in range(steps):
        pre = context_state(ctx)
        st = device_step(ctx, timer)
        post = context_state(ctx)
        counts = (st["density_iterations"], st["divergence_iterations"])
        out = restate_step(ref, pre, post, st["dt_prev"], st["dt"], counts, (bool(st["warmstart_density"]), bool(st["warmstart_divergence"])))
        iterating += counts[0] > 1 or counts[1] > 1
        for avgs, conv, tol, scale in ((out["avgs_density"], ref.density_converged, MAX_AVG_DENSITY_ERROR, st["dt"] / ref.rho0),
                                       (out["avgs_divergence"], ref.divergence_converged, MAX_DIVERGENCE_ERROR, st["dt"])):
            for i, a in enumerate(avgs):
                want = i == len(avgs) - 1
                if conv(a, st["dt"]) != want:
                    assert abs(a * scale - tol) <= STEP_TOL * tol, (i, len(avgs), a * scale, tol)
                    close += 1
    assert iterating >= 5 and close <= 2, (iterating, close)


@pytest.mark.parametrize("kind", [KERNEL_WENDLAND, KERNEL_POLY6, KERNEL_SPIKY], ids=["wendland", "poly6", "spiky"])
def test_update_densities_kernels(kind):
    """sphx_update_densities(kind): the WCSPH density path (Poly6, Spiky) and the DFSPH one (Wendland C2)."""
    ref = restatement()
    bounds = Bounds()
    for name in ("dam_break", "spray", "dense_cluster"):
        pos, vel, boundary = cpu.SCENES[name][0]()
        if name == "dam_break":  # compressed: densities above rho0
            pos = ((pos - pos.mean(0)) * np.float32(0.8) + pos.mean(0)).astype(np.float32)
        ctx = y.SphxContext()
        ctx.set_boundary(boundary)
        ctx.upload(pos, vel)
        ctx.update_neighborhood()
        ctx.update_densities(kind)
        s = context_state(ctx)
        sl = ref.slots(s["counts"], s["lists"], len(s["pos"]))
        rho, m = ref.update_densities(_combined(s), sl, kind)
        assert (rho > ref.rho0).sum() > 10
        bounds.check("density", s["density"], rho, m, sl.n_total, "density", s["ids"], f"{name} kind {kind}")
        ctx.close()
    print(bounds.report())
    bounds.assert_within()


def test_sixteen_million_sampled():
    """configs[2] (the bench scene, 16 M particles): two steps from t = 0 at fixed (3, 2) iterations, then the densities and alpha
    of a seeded sample of 2^16 particles against the restatement on the device's lists (the whole list array is downloaded), the
    third step's vmax against the float64 maximum over all particles (chunked), and — from that state, in a tile context over the
    whole domain — the prediction, one density iteration, the advection, the re-grid and one divergence iteration on the sample."""
    pos, boundary = dam_break(float(np.sqrt(16.0e6 / 4050.0)))
    assert 15_900_000 < len(pos) < 16_100_000
    ctx = y.SphxContext(y.default_params(fixed_iterations=(3, 2)))
    ctx.set_boundary(boundary)
    ctx.upload(pos)
    del pos
    timer = y.TimeManager()
    for _ in range(2):
        device_step(ctx, timer)
    s = context_state(ctx)
    n = len(s["pos"])
    ref = restatement()
    X = _combined(s)
    rows = np.random.default_rng(16).choice(n, 1 << 16, replace=False)
    sl = ref.slots(s["counts"], s["lists"], n, rows)
    bounds = Bounds()
    rho, m = ref.update_densities(X, sl)
    bounds.check("density", s["density"][rows], rho, m, sl.n_total, "density", s["ids"][rows], "16 M")
    alpha, m = ref.compute_alpha_factors(X, sl)
    bounds.check("alpha", s["alpha"][rows], alpha, m, sl.n_total, "alpha", s["ids"][rows], "16 M")
    dt_prev = float(np.float32(timer.simulation_step()))
    vmax = ctx.step_begin(timer.simulation_step())
    best, best_m, nmax = 0.0, 0.0, 0
    for c0 in range(0, n, 1 << 20):
        slc = ref.slots(s["counts"], s["lists"], n, np.arange(c0, min(n, c0 + (1 << 20))))
        acc, acc_m = ref.nonpressure(X, s["vel"], s["density"], slc, dt_prev)
        v, vm = ref.max_velocity_sq(s["vel"][slc.rows], acc, acc_m, dt_prev)
        best, best_m, nmax = max(best, v), max(best_m, vm), max(nmax, int(slc.n_total.max()))
    bounds.check("vmax_sq", [np.float32(vmax) ** 2], [best], [best_m], [nmax], "vmax_sq", None, "16 M")
    ctx.close()
    pos, vel = s["pos"], s["vel"]
    del s, X, sl
    # one density and one divergence iteration, sub-step by sub-step, on the same sample (a tile context over the whole domain)
    b = GpuTileBackend(y.SphxContext(), own_stream=False)
    single_tile(b, pos, vel, boundary)
    del pos, vel
    run_and_check(b, make_plan(1, (1, 1), dts=((dt_prev, dt_prev),)), ref, bounds, "16 M", rows)
    b.ctx.close()
    print(bounds.report())
    bounds.assert_within()
