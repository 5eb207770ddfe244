"""The device's WCSPH step and its physical viscosity model against the float64 restatement of the Rust sources
(tests/dfsph_reference64.py; the CPU counterpart and the reasons are in tests/test_wcsph_reference64.py).

(1) SphxContext.wcsph_step_begin / _finish, both models, over the scenes and sizes of the CPU module: every step recorded (the
state before it, the state between the two phases with the accelerations, lists and sorted boundary, the velocities after it) and
restated from the state before it within |dev - ref| <= C (n + K) 2^-24 M (tests/wcsph_lockstep.py).  (2) The same under the A/B
switches and list formats, on one context of 64 800 particles, sampled rows.  (3) The slot rule of the accelerations
(wscsph.rs:122-129).  (4) GpuTileBackend with the physical model through the DFSPH lock-step plan, plain and fused.  (5) One WCSPH
step and one DFSPH-physical trace per parameter set of tests/constants_scenes.py.  (6) Every mutant is rejected on device data.
(7) Downloading between the two WCSPH phases changes nothing.

Measured worst ratios |device - restatement| / bound on an MI355X over every case of this module (the device is bit-equal with the
fp32 chain of the CPU module, so the figures of shared cases agree to the last digit):
    leapfrog_position 0.135, leapfrog_velocity 0.179, density 0.022, accel 0.0098, vmax_sq 0.018, vmax_sq_own 0.275,
    velocity 0.013, leapfrog2 0.217; DFSPH with the physical model, plain and fused: predict 0.085, vmax_sq 0.015, density 0.144,
    position 0.122, alpha 0.053, velocity 0.070, k 0.015, residual_sum 0.0022.
Smallest excess of a mutant on device data: the boundary force scaled by 1.001, 26 x the bound."""
import numpy as np
import pytest
import constants_scenes as cs
import test_dfsph_reference64 as cpu
import test_wcsph_reference64 as wc
from dfsph_lockstep import Bounds, check_trace, make_plan, membership_of_trace, mutant, restatement, run_plan, single_tile
from dfsph_reference64 import PHYSICAL
from wcsph_lockstep import PHYSICAL_MUTANTS, VISCOSITY_MUTANTS, WCSPH_MUTANTS, WcsphRun, check_step

import yasph2d_amd as y
from tiles_reference import GpuTileBackend

pytestmark = pytest.mark.gpu

H = cpu.H
MODELS = wc.MODELS
STEPS = 4
SCENES = dict(wc.SCENES)
SCENES["n2"] = lambda: cpu.sized(2)
del SCENES["n1024"]  # (the sizes the comparison is asked at: 1, 2, 63, 64, 65, 255, 256, 257, 1023, 1025, 4097)


def device_run(params, scene, diameter=np.float32(0.01), reserve=None):
    ctx = y.SphxContext(params)
    pos, vel, boundary = scene
    if reserve is not None:
        ctx._chk(ctx.L.sphx_reserve(ctx.h, reserve))
    if len(boundary):
        ctx.set_boundary(boundary)
    ctx.upload(pos, vel)
    return WcsphRun(ctx, diameter)


_records = {}


def device_records(name, model):
    if (name, model) not in _records:
        params = wc.model_params(*MODELS[model])
        run = device_run(params, SCENES[name]())
        _records[name, model] = ([run.step() for _ in range(STEPS)], params)
        run.impl.close()
    return _records[name, model]


@pytest.mark.parametrize("model", list(MODELS))
@pytest.mark.parametrize("name", list(SCENES))
def test_device_wcsph_matches_float64_restatement(name, model):
    recs, params = device_records(name, model)
    wc.check_records(recs, restatement(params), f"{name} {model}", membership=not name.startswith("lattice_at_h"))
    if name not in wc.MUTANT_SCENES:
        del _records[name, model]


@pytest.mark.parametrize("model", list(MODELS))
def test_device_wcsph_with_the_capacity_equal_to_an_odd_count(model):
    """sphx_reserve(4097) and 4097 particles: the last workgroup and the last 64-particle list slice are ragged and nothing lies
    behind them."""
    params = wc.model_params(*MODELS[model])
    run = device_run(params, cpu.sized(4097), reserve=4097)
    wc.check_records([run.step() for _ in range(3)], restatement(params), f"n4097 reserved {model}")
    run.impl.close()


@pytest.mark.parametrize("mu", wc.MUS)
def test_device_wcsph_at_other_viscosities(mu):
    params = wc.model_params(PHYSICAL, mu)
    run = device_run(params, wc.compressed_block())
    wc.check_records([run.step() for _ in range(3)], restatement(params), f"compressed_block mu {mu}")
    run.impl.close()


# ----------------------------------------------------------------------------------------------- switches and list formats, 64 800
def compressed_dam_break(scale=4.0, factor=0.8):
    """test_viscosity_host.wcsph_disturbed at 64 800 particles (more than one XCD chunk of workgroups), compressed to 0.8 x its
    spacing (pressures throughout the bulk, some twenty neighbours) and set down one spacing above the floor (its top row lies at
    y = -0.01); of the boundary only the floor rows are kept (a plate of the scene would cut through the block where it now stands)."""
    pos, vel, boundary = wc.wcsph_disturbed(scale)
    lo = pos.min(0)
    return (np.float32([1.0, 0.0]) + (pos - lo) * np.float32(factor)).astype(np.float32), vel, boundary[boundary[:, 1] < np.float32(0.005)]


SWITCHES = [({"SPHX_QCLAMP": "1"}, None), ({"SPHX_LAZY_TABLE": "0"}, None), ({"SPHX_STREAM_LISTS": "1"}, None), ({"SPHX_XCD_CHUNK": "1"}, None),
            ({}, y.LISTS_32BIT), ({}, 60), ({}, 130)]


@pytest.fixture(scope="module")
def big_scene():
    scene = compressed_dam_break()
    assert len(scene[0]) == 64800
    return scene, np.sort(np.random.default_rng(64800).choice(64800, 4096, replace=False))


@pytest.mark.parametrize("model", list(MODELS))
@pytest.mark.parametrize("env,span", SWITCHES, ids=lambda v: (",".join(f"{k}={x}" for k, x in v.items()) or "default") if isinstance(v, dict)
                         else f"span{v}")
def test_device_wcsph_under_switches(monkeypatch, big_scene, env, span, model):
    """k_wcsph_accel's in-window, wide-wavefront and gather paths and both sqrt_dist forms: one step, the lists of 4096 sampled
    particles walked, everything that needs no list compared for all 64 800."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    params = wc.model_params(*MODELS[model])
    if span is not None:
        params.list_span_limit = span
    scene, rows = big_scene
    run = device_run(params, scene)
    rec = run.step()
    run.impl.close()
    bounds = check_step(rec, restatement(params), Bounds(), f"64800 {env} {span} {model}", rows)
    print(f"\n64800 {env} {span} {model}: worst ratios\n{bounds.report()}")
    bounds.assert_within()
    mid = rec["mid"]
    assert (mid["density"][rows] > np.float32(101.0)).sum() > 1000 and (mid["counts"][rows, 1] > mid["counts"][rows, 0]).sum() > 10


# ------------------------------------------------------------------------------------------------------------------ the slot rule
def test_device_accelerations_are_slot_bound():
    """wscsph.rs:122-129 on the device, as tests/test_wcsph_reference64.py::test_accelerations_are_slot_bound states it for the chain:
    zero accelerations after clear_cached (alone, and followed by an upload of another count); an upload of more particles alone
    keeps the held slots and zeroes the new ones."""
    pos, vel, boundary = wc.compressed_block()
    params = wc.model_params("xsph")
    run = device_run(params, (pos, vel, boundary))
    ref = restatement(params)
    bounds = Bounds()
    for _ in range(2):
        check_step(run.step(), ref, bounds, "warm")
    held = run.impl.download_accel()
    run.clear_cached()
    rec = run.step()
    check_step(rec, ref, bounds, "after clear_cached")
    stale = dict(rec, held=len(pos), pre=dict(rec["pre"], accel=held))
    assert check_step(stale, ref, Bounds()).max_ratio() > 1.0
    d = run.impl.download()
    extra = (d["pos"][:37] + np.float32([0.0, 0.5])).astype(np.float32)
    run.impl.upload(np.concatenate([d["pos"], extra]), np.concatenate([d["vel"], np.zeros_like(extra)]))
    rec = run.step()
    assert rec["held"] == len(pos) and len(rec["mid"]["pos"]) == len(pos) + 37
    check_step(rec, ref, bounds, "after growth")
    assert check_step(dict(rec, held=0), ref, Bounds()).max_ratio() > 1.0
    run.clear_cached()
    d = run.impl.download()
    run.impl.upload(d["pos"][:-50], d["vel"][:-50])
    rec = run.step()
    assert rec["held"] == 0
    check_step(rec, ref, bounds, "after clear_cached and an upload of another count")
    run.impl.close()
    print(bounds.report())
    bounds.assert_within()


# --------------------------------------------------------------------------------------------------- DFSPH with the physical model
def physical_device_trace(params, scene, plan):
    b = GpuTileBackend(y.SphxContext(params), own_stream=False)
    single_tile(b, *scene)
    trace = run_plan(b, plan)
    b.ctx.close()
    return trace


def check_physical(trace, params, where, particle_density=10000.0, h=H, grid_min=(-100.0, -100.0)):
    bounds = check_trace(trace, restatement(params, particle_density), Bounds(), where)
    print(f"\n{where}: worst ratios\n{bounds.report()}")
    bounds.assert_within()
    membership_of_trace(trace, h, grid_min=grid_min)


_traces = {}


def physical_trace(name, fuse):
    if (name, fuse) not in _traces:
        make, steps, fixed = cpu.SCENES[name]
        params = wc.model_params(PHYSICAL, 0.01)
        plan = make_plan(steps, fixed, fuse_predict=fuse, regrid="fused" if fuse else "plain")
        _traces[name, fuse] = (physical_device_trace(params, make(), plan), params)
    return _traces[name, fuse]


@pytest.mark.parametrize("fuse", [False, True], ids=["plain", "fused"])
@pytest.mark.parametrize("name", ["dam_break", "spray", "n1", "n63", "n1025", "n4097"])
def test_device_dfsph_physical_substeps_match_float64_restatement(name, fuse):
    trace, params = physical_trace(name, fuse)
    check_physical(trace, params, f"{name} physical {'fused' if fuse else 'plain'}")


# ------------------------------------------------------------------------------------------------- away from the app's constants
@pytest.mark.parametrize("model", list(MODELS))
@pytest.mark.parametrize("name", cs.SET_IDS)
def test_device_wcsph_away_from_the_apps_constants(name, model):
    params = wc.model_params(*MODELS[model], name=name)
    run = device_run(params, cs.scene(name), cs.diameter(name))
    rec = run.step()
    run.impl.close()
    wc.check_records([rec], restatement(params, cs.particle_density(name)), f"{name} {model}", float(cs.properties(name)["smoothing_length"]),
                     cs.SETS[name][4])


@pytest.mark.parametrize("name", cs.SET_IDS)
def test_device_dfsph_physical_away_from_the_apps_constants(name):
    params = wc.model_params(PHYSICAL, 0.01, name)
    plan = make_plan(1, (2, 2), dt_scale=float(cs.spacing(name)) / 0.01)
    trace = physical_device_trace(params, cs.scene(name), plan)
    check_physical(trace, params, f"{name} physical", cs.particle_density(name), float(cs.properties(name)["smoothing_length"]), cs.SETS[name][4])


# ---------------------------------------------------------------------------------------------------------------------- mutants
@pytest.mark.parametrize("cls", VISCOSITY_MUTANTS + PHYSICAL_MUTANTS + WCSPH_MUTANTS, ids=lambda c: c.__name__)
def test_mutant_is_rejected_on_device_wcsph_data(cls):
    for model in ["physical"] if cls in PHYSICAL_MUTANTS else list(MODELS):
        ratio = wc.mutant_ratio(cls, [device_records(name, model) for name in wc.MUTANT_SCENES])
        print(f"\n{cls.__name__} {model}: {ratio:.3g} x the bound")
        assert ratio > 1.0, f"mutant '{cls.__doc__}' passes the WCSPH comparison on device data with {model} (ratio {ratio:.3g})"


@pytest.mark.parametrize("cls", VISCOSITY_MUTANTS + PHYSICAL_MUTANTS, ids=lambda c: c.__name__)
def test_viscosity_mutant_is_rejected_on_device_dfsph_data(cls):
    ratio = 0.0
    for name in ("dam_break", "spray"):
        for fuse in (False, True):
            trace, params = physical_trace(name, fuse)
            ratio = max(ratio, check_trace(trace, mutant(cls, params), Bounds(), name).max_ratio())
    print(f"\n{cls.__name__}: {ratio:.3g} x the bound")
    assert ratio > 1.0, f"mutant '{cls.__doc__}' passes the DFSPH comparison on device data (ratio {ratio:.3g})"


# -------------------------------------------------------------------------------------------------------------------- downloads
@pytest.mark.parametrize("model", list(MODELS))
def test_downloads_between_the_phases_change_nothing(model):
    params = wc.model_params(*MODELS[model])
    out = []
    for record in (True, False):
        run = device_run(params, wc.compressed_block())
        for _ in range(STEPS):
            run.step(record=record)
        out.append((run.impl.download(), run.timer.simulation_step_ns()))
        run.impl.close()
    (a, ta), (b, tb) = out
    assert ta == tb
    for k in ("ids", "pos", "vel", "density"):
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k


def test_half_step_download_answers_between_the_wcsph_phases_only():
    """sphx_debug_download_wcsph_half_step: refused before a step, inside a DFSPH step and after the WCSPH step; sphx_download stays
    refused inside the WCSPH step; positions, densities and ids of the half step are those after the step."""
    from yasph2d_amd import _lib

    def refused(fn):
        with pytest.raises(y.SphxError) as e:
            fn()
        assert e.value.code == _lib.ERR_NOT_READY

    pos, vel, boundary = wc.compressed_block()
    ctx = y.SphxContext()
    ctx.set_boundary(boundary)
    ctx.upload(pos, vel)
    refused(ctx.download_wcsph_half_step)
    ctx.step_begin(np.float32(1e-4))
    refused(ctx.download_wcsph_half_step)
    ctx.step_finish(np.float32(1e-4))
    ctx.wcsph_step_begin(np.float32(1e-4))
    refused(ctx.download)
    half = ctx.download_wcsph_half_step()
    ctx.wcsph_step_finish(np.float32(1e-4))
    refused(ctx.download_wcsph_half_step)
    d = ctx.download()
    ctx.close()
    for k in ("pos", "density", "ids"):
        assert np.array_equal(half[k].view(np.uint32), d[k].view(np.uint32)), k
    assert not np.array_equal(half["vel"], d["vel"])
