"""WCSPH and the physical viscosity model against the float64 restatement of the Rust sources (tests/dfsph_reference64.py), without
a GPU.

The device's WCSPH step and its physical viscosity are compared bit for bit with the oracle (orc_wcsph_step) and with
tests/viscosity_reference.py — fp32 restatements by the same hand as the kernels.  A misreading of wscsph.rs, physical.rs or
viscosity.rs, or a wrongly derived constant, would sit in all three.  Here that fp32 chain (wcsph_lockstep.ChainWcsph, behind the
begin / finish interface the device offers) runs step by step under the float64 restatement, which derives every constant itself:
each step is restated from the state before it and compared within |dev - ref| <= C (n + K) 2^-24 M (tests/wcsph_lockstep.py; C = 2,
the K entries and their counts in tests/dfsph_lockstep.py).  The DFSPH sub-steps with the physical model
(viscosity_reference.ViscousOracleTileBackend) go through dfsph_lockstep.check_trace, which hands the model on.  Every mutant of the
restatement must be rejected on the same recorded data.

Measured worst ratios |chain - restatement| / bound on a CPU, over every case of this module (both models, the scenes of
tests/test_dfsph_reference64.py, the still lattice, the disturbed dam break, the compressed block, three viscosities and the five
parameter sets; the device's figures are in tests/test_gpu_wcsph_reference64.py):
    leapfrog_position 0.135, leapfrog_velocity 0.179, density 0.022, accel 0.0098, vmax_sq 0.013, vmax_sq_own 0.275,
    velocity 0.013, leapfrog2 0.217; DFSPH with the physical model: predict 0.085, vmax_sq 0.046, density 0.144, position 0.127,
    alpha 0.083, velocity 0.070, k 0.015, residual_sum 0.0022.
Smallest excess of a mutant: the boundary force scaled by 1.001, 26 x the bound; every other one exceeds 100 x."""
import numpy as np
import pytest
import constants_scenes as cs
import test_dfsph_reference64 as cpu
from dfsph_lockstep import Bounds, check_trace, make_plan, mutant, restatement, run_plan, single_tile
from dfsph_reference64 import PHYSICAL, XSPH
from test_viscosity_host import wcsph_disturbed
from wcsph_lockstep import (PHYSICAL_MUTANTS, VISCOSITY_MUTANTS, WCSPH_MUTANTS, ChainWcsph, WcsphRun, check_step, membership_of_step)

import yasph2d_amd as y

H = cpu.H
MUS = [1.0016e-3, 0.01, -0.005]
MODELS = {"xsph": (XSPH, None), "physical": (PHYSICAL, 0.01)}
STEPS = 3


def compressed_block(n=900, factor=0.93, seed=11):
    """A jittered lattice block at 0.93 x the particle spacing over a floor, with velocity jumps: Poly6 densities above rho0 in the
    bulk (nonzero pressures that differ between neighbours), clamped to rho0 at the rim, the lowest row within reach of the boundary
    force."""
    pos, vel, boundary = cs.scene((2.0, 1.0e4, 100.0, cs.DEFAULT_GRAVITY, cs.DEFAULT_GRID_MIN), n, seed=seed, velocity_scale=20.0)
    o = np.array(cs.ORIGIN, np.float32)
    return (o + (pos - o) * np.float32(factor)).astype(np.float32), vel, boundary


def grazing_pairs(count=6, seed=5):
    """Isolated pairs that pass the list rule d^2 <= h^2 in fp32 (neighborhood_search.rs:357) while their float64 distance lies
    within an ulp of h: `count` pairs beyond h (the viscosity Laplacian is negative there, viscosity.rs:45-47 has no r < h test, and
    the Spiky kernel's max(h - r, 0) cuts) and `count` short of it.  Found by a seeded search on the circle around each centre."""
    h = np.float32(H)
    u = float(np.spacing(h))
    rng = np.random.default_rng(seed)
    out = []
    for m in range(2 * count):
        c = np.array([-0.25, 2.0 + 0.125 * m], np.float32)
        th = rng.uniform(0.0, 2.0 * np.pi, 20000)
        pj = (c.astype(np.float64) + float(h) * np.stack([np.cos(th), np.sin(th)], 1)).astype(np.float32)
        d = pj - c
        member = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] <= h * h
        short = float(h) - np.sqrt(((pj.astype(np.float64) - c.astype(np.float64)) ** 2).sum(1))
        ok = member & ((short < 0) if m < count else ((short > 0) & (short < 4 * u)))
        assert ok.any()
        out += [c, pj[int(np.argmax(ok))]]
    return np.array(out, np.float32)


def lattice_at_h_still():
    """test_dfsph_reference64.lattice_at_h with its lattice points and its exact-h pairs at rest, and the grazing pairs, at rest too:
    the first step's leap frog 1 (zero accelerations) leaves them where they are, so the lists of that step hold pairs with h - r
    within a few ulp of zero on both sides and at zero; the twins and the half-spacing rows keep their velocities."""
    pos, vel, boundary = cpu.lattice_at_h()
    vel[:576] = 0
    vel[-20:] = 0
    extra = grazing_pairs()
    return np.concatenate([pos, extra]), np.concatenate([vel, np.zeros_like(extra)]), boundary


SCENES = {k: v[0] for k, v in cpu.SCENES.items()}
SCENES["lattice_at_h_still"] = lattice_at_h_still
SCENES["wcsph_disturbed"] = wcsph_disturbed
SCENES["compressed_block"] = compressed_block
MUTANT_SCENES = ("wcsph_disturbed", "compressed_block", "dense_cluster", "boundary_only")


def model_params(model, coef=None, name=None):
    """The parameter block of a model ("xsph": the block's own epsilon) at the app's constants or at a set of constants_scenes."""
    kw = dict(viscosity="physical", fluid_viscosity=coef) if model == PHYSICAL else {}
    return y.default_params(**kw) if name is None else cs.params(name, **kw)


def coefficient(params):
    return params.fluid_viscosity if params.viscosity_model == y.VISCOSITY_PHYSICAL else params.xsph_epsilon


def chain_run(params, scene, oracle=None, diameter=np.float32(0.01)):
    model = PHYSICAL if params.viscosity_model == y.VISCOSITY_PHYSICAL else XSPH
    impl = ChainWcsph(model, coefficient(params), params, oracle)
    pos, vel, boundary = scene
    if len(boundary):
        impl.set_boundary(boundary)
    impl.upload(pos, vel)
    return WcsphRun(impl, diameter)


_records = {}


def chain_records(name, model):
    """STEPS recorded steps of the fp32 chain on a scene at the app's constants -> (records, parameter block)."""
    if (name, model) not in _records:
        params = model_params(*MODELS[model])
        run = chain_run(params, SCENES[name]())
        _records[name, model] = ([run.step() for _ in range(STEPS)], params)
    return _records[name, model]


def check_records(recs, ref, where, h=H, grid_min=(-100.0, -100.0), membership=True):
    bounds = Bounds()
    for s, rec in enumerate(recs):
        check_step(rec, ref, bounds, f"{where} step {s}")
        if membership:
            membership_of_step(rec, h, grid_min=grid_min)
    print(f"\n{where}: worst ratios\n{bounds.report()}")
    bounds.assert_within()
    return bounds


def test_chain_behind_the_interface_is_the_chain_proven_against_the_oracle():
    """ChainWcsph composes viscosity_reference.wcsph_* as test_viscosity_host.numpy_wcsph_run does (which is bit-equal to
    orc_wcsph_step): the same vmax, dt and state, bit for bit."""
    from test_viscosity_host import numpy_wcsph_run

    pos, vel, boundary = wcsph_disturbed()
    eps = y.default_params().xsph_epsilon
    want, p, v = numpy_wcsph_run(XSPH, eps, pos, vel, boundary, 6)
    run = chain_run(y.default_params(), (pos, vel, boundary))
    got = []
    for _ in range(6):
        rec = run.step(record=False)
        got.append((np.float32(rec["vmax"]), run.timer.simulation_step_ns()))
    assert got == want
    d = run.impl.download()
    assert np.array_equal(d["pos"].view(np.uint32), p.view(np.uint32)) and np.array_equal(d["vel"].view(np.uint32), v.view(np.uint32))


@pytest.mark.parametrize("model", list(MODELS))
@pytest.mark.parametrize("name", list(SCENES))
def test_wcsph_chain_matches_float64_restatement(name, model):
    """(No brute-force membership check on the lattice of spacing h once leap frog 1 has moved it: a pair a hair closer than h whose
    cell coordinates (pos - grid_min) / h round to cells two apart is not found by the reference's 3 x 3 cell search,
    neighborhood_search.rs:193-194, and the brute-force rule knows nothing of cells.)"""
    recs, params = chain_records(name, model)
    check_records(recs, restatement(params), f"{name} {model}", membership=not name.startswith("lattice_at_h"))


@pytest.mark.parametrize("mu", MUS)
def test_wcsph_chain_at_other_viscosities(mu):
    params = model_params(PHYSICAL, mu)
    run = chain_run(params, compressed_block())
    check_records([run.step() for _ in range(STEPS)], restatement(params), f"compressed_block mu {mu}")


@pytest.mark.parametrize("model", list(MODELS))
@pytest.mark.parametrize("name", cs.SET_IDS)
def test_wcsph_chain_away_from_the_apps_constants(name, model):
    """At h = 0.0025 one step only: the block flies apart there (README, "Found there")."""
    params = model_params(*MODELS[model], name=name)
    run = chain_run(params, cs.scene(name), cs.oracle(name), cs.diameter(name))
    recs = [run.step() for _ in range(1 if name == "tiny" else STEPS)]
    check_records(recs, restatement(params, cs.particle_density(name)), f"{name} {model}", float(cs.properties(name)["smoothing_length"]),
                  cs.SETS[name][4])


# ---------------------------------------------------------------------------------------------------- DFSPH with the physical model
_traces = {}


def physical_trace(name, mu=0.01, constants=None):
    """The DFSPH sub-step plan of test_dfsph_reference64 on the oracle's tile backend with the non-pressure pass and the prediction
    of the physical model in fp32 numpy -> (trace, parameter block)."""
    from viscosity_reference import ViscousOracleTileBackend

    key = (name, mu, constants)
    if key not in _traces:
        if constants is None:
            make, steps, fixed = cpu.SCENES[name]
            params = model_params(PHYSICAL, mu)
            b = ViscousOracleTileBackend(PHYSICAL, mu)
            plan = make_plan(steps, fixed)
            pos, vel, boundary = make()
        else:
            params = model_params(PHYSICAL, mu, constants)
            b = ViscousOracleTileBackend(PHYSICAL, mu, params, cs.oracle(constants))
            plan = make_plan(2, (2, 2), dt_scale=float(cs.spacing(constants)) / 0.01)
            pos, vel, boundary = cs.scene(constants)
        single_tile(b, pos, vel, boundary)
        _traces[key] = (run_plan(b, plan), params)
    return _traces[key]


def check_physical_trace(trace, params, where, particle_density=10000.0):
    bounds = check_trace(trace, restatement(params, particle_density), Bounds(), where)
    print(f"\n{where}: worst ratios\n{bounds.report()}")
    bounds.assert_within()


@pytest.mark.parametrize("name", list(cpu.SCENES))
def test_dfsph_physical_substeps_match_float64_restatement(name):
    check_physical_trace(*physical_trace(name), f"{name} physical")


@pytest.mark.parametrize("mu", [MUS[0], MUS[2]])
def test_dfsph_physical_substeps_at_other_viscosities(mu):
    check_physical_trace(*physical_trace("dam_break", mu), f"dam_break mu {mu}")


@pytest.mark.parametrize("name", cs.SET_IDS)
def test_dfsph_physical_substeps_away_from_the_apps_constants(name):
    check_physical_trace(*physical_trace(None, 0.01, name), f"{name} physical", cs.particle_density(name))


def test_check_trace_takes_the_model_as_an_argument():
    """A restatement made for XSPH checks a physical trace when the model is handed to check_trace, and fails it when it is not."""
    trace, params = physical_trace("dam_break")
    ref = restatement()
    assert ref.model[0] == XSPH
    check_trace(trace, ref, Bounds(), "dam_break", model=(PHYSICAL, params.fluid_viscosity)).assert_within()
    assert check_trace(trace, ref, Bounds(), "dam_break").max_ratio() > 1.0


# ------------------------------------------------------------------------------------------------------------------------ edges
def test_scenes_reach_the_edges():
    """The inputs hold what the comparison is there for (asserted on the recorded states between the two phases)."""
    u = float(np.spacing(np.float32(H)))
    # list members with h - r within a few ulp of zero on both sides (float64 distance of the fp32 positions)
    mid = chain_records("lattice_at_h_still", "physical")[0][0]["mid"]
    X = np.concatenate([mid["pos"], mid["boundary"]]).astype(np.float64)
    start = np.concatenate([[0], np.cumsum(mid["counts"][:, 1].astype(np.int64))])
    i = np.repeat(np.arange(len(mid["pos"])), mid["counts"][:, 1])
    k = np.arange(len(i)) - start[i]
    dyn = k < mid["counts"][i, 0]
    j = np.where(dyn, mid["lists"], len(mid["pos"]) + mid["lists"].astype(np.int64))
    d = float(np.float32(H)) - np.sqrt(((X[j] - X[i]) ** 2).sum(1))
    assert ((d > 0) & (d < 4 * u)).any() and ((d < 0) & (d > -4 * u)).any() and (d == 0).any(), (d[np.abs(d) < 8 * u] / u).tolist()
    # densities clamped to rho0 (zero pressure) and above it; neighbouring pressures that differ
    mid = chain_records("compressed_block", "xsph")[0][0]["mid"]
    rho0 = np.float32(100.0)
    assert (mid["density"] == rho0).sum() > 20 and (mid["density"] > rho0 * np.float32(1.01)).sum() > 100
    # particles with static neighbours and with none
    stat = mid["counts"][:, 1] - mid["counts"][:, 0]
    assert (stat > 0).sum() > 10 and (stat == 0).sum() > 100
    mid = chain_records("boundary_only", "xsph")[0][0]["mid"]
    assert (mid["counts"][:, 0] == 0).all() and (mid["counts"][:, 1] > 0).all()
    # capped lists
    assert (chain_records("dense_cluster", "xsph")[0][0]["mid"]["counts"][:, 1] == 64).any()
    # a neighbour pair with equal velocities and one with different velocities
    mid = chain_records("wcsph_disturbed", "physical")[0][0]["mid"]
    start = np.concatenate([[0], np.cumsum(mid["counts"][:, 1].astype(np.int64))])
    i = np.repeat(np.arange(len(mid["pos"])), mid["counts"][:, 1])
    dyn = (np.arange(len(i)) - start[i]) < mid["counts"][i, 0]
    same = (mid["vel"][mid["lists"][dyn]] == mid["vel"][i[dyn]]).all(1)
    assert same.sum() > 100 and (~same).sum() > 100
    # the timer changed dt inside a step (leap frog 2's dt is not leap frog 1's), and accelerations are held from the second step on
    recs = chain_records("wcsph_disturbed", "physical")[0]
    assert all(r["dt2"] != r["dt"] for r in recs) and [r["held"] for r in recs] == [0] + [len(mid["pos"])] * (STEPS - 1)
    assert np.abs(recs[1]["pre"]["accel"]).max() > 1.0


def test_accelerations_are_slot_bound():
    """wscsph.rs:122-129: clear_cached_data empties `accellerations`, resize keeps the held slots and fills up with zeros.  The
    restatement predicts leap frog 1 from the count the runner keeps; a step after clear_cached starts from zero accelerations, and
    so does the first step after clear_cached and an upload of another count; an upload of more particles alone keeps the old slots."""
    pos, vel, boundary = compressed_block()
    params = model_params(XSPH)
    run = chain_run(params, (pos, vel, boundary))
    ref = restatement(params)
    bounds = Bounds()
    for _ in range(2):
        check_step(run.step(), ref, bounds, "warm")
    held = run.impl.download_accel()
    run.clear_cached()
    rec = run.step()
    assert rec["held"] == 0
    check_step(rec, ref, bounds, "after clear_cached")
    stale = dict(rec, held=len(pos), pre=dict(rec["pre"], accel=held))
    assert check_step(stale, ref, Bounds()).max_ratio() > 1.0  # (held accelerations would have shown)
    d = run.impl.download()
    extra = (d["pos"][:37] + np.float32([0.0, 0.5])).astype(np.float32)
    run.impl.upload(np.concatenate([d["pos"], extra]), np.concatenate([d["vel"], np.zeros_like(extra)]))
    rec = run.step()
    assert rec["held"] == len(pos) and len(rec["mid"]["pos"]) == len(pos) + 37
    check_step(rec, ref, bounds, "after growth")
    assert check_step(dict(rec, held=0), ref, Bounds()).max_ratio() > 1.0  # (the old slots kept theirs)
    run.clear_cached()
    d = run.impl.download()
    run.impl.upload(d["pos"][:-50], d["vel"][:-50])
    rec = run.step()
    assert rec["held"] == 0
    check_step(rec, ref, bounds, "after clear_cached and an upload of another count")
    print(bounds.report())
    bounds.assert_within()


# ---------------------------------------------------------------------------------------------------------------------- mutants
def mutant_ratio(cls, records):
    ratio = 0.0
    for recs, params in records:
        b = Bounds()
        for rec in recs:
            check_step(rec, mutant(cls, params), b)
        ratio = max(ratio, b.max_ratio())
    return ratio


@pytest.mark.parametrize("cls", VISCOSITY_MUTANTS + PHYSICAL_MUTANTS + WCSPH_MUTANTS, ids=lambda c: c.__name__)
def test_mutant_is_rejected_on_wcsph_chain_data(cls):
    models = ["physical"] if cls in PHYSICAL_MUTANTS else list(MODELS)
    for model in models:  # each model's data alone must reject it
        ratio = mutant_ratio(cls, [chain_records(name, model) for name in MUTANT_SCENES])
        print(f"\n{cls.__name__} {model}: {ratio:.3g} x the bound")
        assert ratio > 1.0, f"mutant '{cls.__doc__}' passes the WCSPH comparison with {model} (ratio {ratio:.3g})"


@pytest.mark.parametrize("cls", VISCOSITY_MUTANTS + PHYSICAL_MUTANTS, ids=lambda c: c.__name__)
def test_viscosity_mutant_is_rejected_on_dfsph_physical_data(cls):
    ratio = 0.0
    for name in ("dam_break", "spray", "dense_cluster"):
        trace, params = physical_trace(name)
        ratio = max(ratio, check_trace(trace, mutant(cls, params), Bounds(), name).max_ratio())
    print(f"\n{cls.__name__}: {ratio:.3g} x the bound")
    assert ratio > 1.0, f"mutant '{cls.__doc__}' passes the DFSPH comparison (ratio {ratio:.3g})"
