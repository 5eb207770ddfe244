"""The oracle away from the reference app's constants (tests/constants_scenes.py: five parameter sets), without a GPU.

(1) The oracle's DFSPH sub-steps against the float64 restatement built for each set, lock-step, inside the unchanged round-off bound
of tests/dfsph_lockstep.py — the oracle derives its kernel constants (1/h, the normalisers, the mass) from the set in fp32, the
restatement derives its own in float64 from the same inputs; at h = 0.02 the two were known to agree, here they meet at h = 0.03,
0.04, 0.01, 0.0025000002 and 0.18033393.  Every mutant of the restatement is still rejected at the set `fine`.
(2) The runs the GPU tests (tests/test_gpu_constants.py) compare with the device do what they are there for, in the oracle alone:
finite velocities, no would-be panic, divergence loops of more than one iteration, warm starts, the iteration caps.

Worst ratio |oracle - restatement| / bound per set (1500-particle scene, 3 steps at fixed (3, 2)), next to the <= 0.123 of the
scenes of tests/test_dfsph_reference64.py at the default constants:
    wide 0.112 (position), coarse_water 0.115 (position), fine 0.112 (position), tiny 0.081 (predict), odd 0.113 (position)."""
import numpy as np
import pytest
import constants_scenes as cs
from dfsph_lockstep import MUTANTS, Bounds, check_trace, make_plan, membership_of_trace, mutant, restatement, run_plan, single_tile

ADAPTIVE_STEPS = 40     # tests/test_gpu_constants.py, DFSPH adaptive
FIXED_STEPS = 12        # ... fixed (2, 2)
WCSPH_STEPS = 25
KNOB_STEPS = 20         # xsph_epsilon 0.0 / 0.5 at coarse_water
CAP_STEPS = 30          # tolerances (1e-8, 7, 1e-6, 5) at coarse_water
CAP_TOLERANCES = (1.0e-8, 7, 1.0e-6, 5)
CAP_VELOCITY_SCALE = 0.5  # the scene's own: the oracle reaches both caps with it (test_caps_are_reached_in_the_oracle)
FEATURE_STEPS = 10      # the state the feature tests (sampling, fields, render, statistics, save, tiles) start from
SATURATED_N = 300


def dt_scale(name):
    """make_plan's dts and the fixed 50 us step were chosen at spacing 0.01."""
    return float(cs.spacing(name)) / 0.01


def fixed_step_ns(name):
    return int(round(50_000 * dt_scale(name)))


def oracle_with_scene(name, n=cs.STEP_N, velocity_scale=0.5):
    o = cs.oracle(name)
    pos, vel, boundary = cs.scene(name, n, velocity_scale=velocity_scale)
    o.set_boundary(boundary)
    o.set_particles(pos, vel)
    return o


_traces = {}


def oracle_trace(name):
    if name not in _traces:
        from tile_oracle_backend import OracleTileBackend

        pos, vel, boundary = cs.scene(name)
        b = OracleTileBackend(cs.oracle(name), h=float(cs.properties(name)["smoothing_length"]), grid_min=cs.SETS[name][4])
        single_tile(b, pos, vel, boundary)
        _traces[name] = run_plan(b, make_plan(3, (3, 2), dt_scale=dt_scale(name)))
    return _traces[name]


def test_sets_are_what_the_table_says():
    """h, m and the radius of every set as the oracle derives them, and the two rounding edges the sets were chosen for."""
    want = {"wide": (0.03, 0.01, 0.005), "coarse_water": (0.04, 0.4, 0.01), "fine": (0.01, 0.024925, 0.0025), "tiny": (0.0025000002, 1.0e-6, 0.0005),
            "odd": (0.18033393, 0.030081302, 0.04508348)}
    for name in cs.SET_IDS:
        p, q = cs.oracle(name).properties(), cs.properties(name)
        for k in p:
            assert np.float32(p[k]) == np.float32(q[k]), (name, k, p[k], q[k])
        lib = cs.params(name)
        assert (np.float32(lib.smoothing_length), np.float32(lib.particle_mass), np.float32(lib.particle_radius), np.float32(lib.fluid_density)) == (
            p["smoothing_length"], p["particle_mass"], p["particle_radius"], p["fluid_density"]), name
        assert (p["smoothing_length"], p["particle_mass"], p["particle_radius"]) == tuple(np.float32(x) for x in want[name]), (name, p)
        assert tuple(lib.gravity) == tuple(np.float32(x) for x in cs.SETS[name][3]) and tuple(lib.grid_min) == cs.SETS[name][4]
    assert cs.properties("tiny")["smoothing_length"] != np.float32(0.0025)
    h = cs.properties("odd")["smoothing_length"]
    assert h * (np.float32(1.0) / h) == np.float32(0.99999994)
    for name in cs.SET_IDS:  # the origin is no lattice point of the cell grid
        h, gm = cs.properties(name)["smoothing_length"], np.array(cs.SETS[name][4], np.float32)
        c = (np.array(cs.ORIGIN, np.float32) - gm) * (np.float32(1.0) / h)
        assert (np.abs(c - np.round(c)) > 0.01).all() and (c > 2).all() and (c < 65534).all(), (name, c)


@pytest.mark.parametrize("name", cs.SET_IDS + ["default", "saturated"])
def test_derived_kernel_constants_agree_bit_for_bit(name):
    """1/h, h^2 and the Wendland, Poly6 and Spiky normalisers as the oracle's kernels derive them from h (orc_kernel_constants) against
    the numpy restatements of sphx_create's derivation that the feature references use (sample_reference, fields_reference,
    viscosity_reference): fp32, bit for bit.  The round-off bound of the lock-step comparison cannot see one ulp in a constant; this can."""
    import ctypes as C

    import fields_reference as fr
    import sample_reference as sr
    import viscosity_reference as vr
    from oracle.oracle import lib

    import yasph2d_amd as y

    p = y.default_params() if name == "default" else cs.params(cs.SATURATED if name == "saturated" else name)
    h = np.float32(p.smoothing_length)
    got = np.zeros((3, 3), np.float32)
    for kind in range(3):
        lib().orc_kernel_constants(kind, h, got[kind].ctypes.data_as(C.c_void_p))
    S, Fd, V = sr.Constants(p), fr.Constants(p), vr.Constants(p)
    want = {"w_hinv": (got[0, 0], S.w_hinv, Fd.w_hinv, S.cell_inv), "w_norm": (got[0, 1], S.w_norm), "w_ngrad": (got[0, 2], Fd.w_ngrad),
            "p6_hsq": (got[1, 0], S.p6_hsq, V.p6_hsq, S.radius_sq), "p6_norm": (got[1, 1], S.p6_norm, V.p6_norm),
            "sp_norm": (got[2, 1], S.sp_norm, V.sp_norm), "sp_ngrad": (got[2, 2], V.sp_ngrad)}
    for k, vals in want.items():
        bits = {np.float32(v).view(np.uint32).item() for v in vals}
        assert len(bits) == 1 and np.isfinite(vals[0]) and vals[0] > 0, (name, k, [repr(np.float32(v)) for v in vals])
    assert (V.m, V.rho0) == (np.float32(p.particle_mass), np.float32(p.fluid_density))


@pytest.mark.parametrize("name", cs.SET_IDS)
def test_oracle_substeps_match_float64_restatement(name):
    trace = oracle_trace(name)
    bounds = check_trace(trace, restatement(cs.params(name), cs.particle_density(name)), Bounds(), name)
    print(f"\n{name}: worst ratios\n{bounds.report()}")
    bounds.assert_within()
    membership_of_trace(trace, float(cs.properties(name)["smoothing_length"]), grid_min=cs.SETS[name][4])


@pytest.mark.parametrize("cls", MUTANTS, ids=lambda c: c.__name__)
def test_mutant_is_rejected_at_fine(cls):
    b = check_trace(oracle_trace("fine"), mutant(cls, cs.params("fine"), cs.particle_density("fine")), Bounds(), "fine")
    print(f"\n{cls.__name__}: {b.max_ratio():.3g} x the bound")
    assert b.max_ratio() > 1.0, f"mutant '{cls.__doc__}' passes the comparison at the set fine (ratio {b.max_ratio():.3g})"


def test_scene_is_built_as_described():
    for name in cs.SET_IDS:
        s = cs.spacing(name)
        for n in cs.CHEAP_N + (cs.STEP_N,):
            pos, vel, boundary = cs.scene(name, n)
            side = int(np.ceil(np.sqrt(n)))
            assert pos.shape == vel.shape == (n, 2) and pos.dtype == vel.dtype == boundary.dtype == np.float32
            assert len(boundary) == 3 * (side + 8)
            assert boundary[:, 0].min() < pos[:, 0].min() - 3.5 * s and boundary[:, 0].max() > pos[:, 0].min() + (side - 1 + 3.5) * s
            gap = pos[:, 1].min() - boundary[:, 1].max()
            assert 0.9 * s < gap < 1.1 * s
            assert 0.3 * s < np.abs(vel).mean() / 0.8 < 0.7 * s  # E|N(0, sigma)| = 0.8 sigma, sigma = 0.5 s


def check_run(stats, o, what):
    """The scene's run does what the GPU comparison needs of it (asserted in the oracle alone)."""
    assert np.isfinite(o.velocities()).all() and np.isfinite(o.positions()).all(), what
    assert not any(s["neighbor_flags"] & 2 for s in stats), what  # the reference would have panicked (neighborhood_search.rs:373)


@pytest.mark.parametrize("name", cs.SET_IDS)
def test_adaptive_runs_reach_the_edges(name):
    """Within the 40 adaptive steps of the GPU test: finite velocities, no would-be panic, a divergence loop of more than one
    iteration, a warm start.  Likewise within the 10 steps the feature tests start from (set fine)."""
    o = oracle_with_scene(name)
    stats = [o.dfsph_step() for _ in range(ADAPTIVE_STEPS)]
    check_run(stats, o, name)
    for upto in (ADAPTIVE_STEPS,) + ((FEATURE_STEPS,) if name == "fine" else ()):
        assert any(s["divergence_iterations"] > 1 for s in stats[:upto]), (name, upto)
        assert sum(s["warmstart_density"] + s["warmstart_divergence"] for s in stats[:upto]) >= 1, (name, upto)


@pytest.mark.parametrize("name", cs.SET_IDS)
def test_fixed_and_wcsph_runs_stay_finite(name):
    o = oracle_with_scene(name)
    o.set_fixed_iterations(2, 2)
    o.timer_fixed(fixed_step_ns(name))
    stats = [o.dfsph_step() for _ in range(FIXED_STEPS)]
    check_run(stats, o, name + " fixed")
    assert sum(s["warmstart_density"] + s["warmstart_divergence"] for s in stats) == 2 * (FIXED_STEPS - 1)
    o = oracle_with_scene(name)
    o.timer_adaptive(2_777_778, 41_667, 0.2)
    stats = [o.wcsph_step() for _ in range(WCSPH_STEPS)]
    check_run(stats, o, name + " wcsph")


@pytest.mark.parametrize("epsilon", [0.0, 0.5])
def test_xsph_epsilon_changes_the_oracle_run(epsilon):
    """orc_set_xsph_epsilon reaches the solver: the run differs from the one at 0.05; setting 0.05 changes nothing."""
    def run(eps):
        o = oracle_with_scene("coarse_water")
        if eps is not None:
            o.set_xsph_epsilon(eps)
        stats = [o.dfsph_step() for _ in range(KNOB_STEPS)]
        check_run(stats, o, eps)
        return o.velocities(), stats

    base, _ = run(None)
    same, _ = run(0.05)
    assert np.array_equal(base.view(np.uint32), same.view(np.uint32))
    other, stats = run(epsilon)
    assert not np.array_equal(base.view(np.uint32), other.view(np.uint32))
    assert any(s["divergence_iterations"] > 1 for s in stats) and sum(s["warmstart_divergence"] for s in stats) >= 1


def test_caps_are_reached_in_the_oracle():
    """Tolerances no loop can meet in 7 / 5 iterations: the counts reach 8 and 6, the cap plus one (dfsph.rs:236,391)."""
    o = oracle_with_scene("coarse_water", velocity_scale=CAP_VELOCITY_SCALE)
    o.set_tolerances(*CAP_TOLERANCES)
    stats = [o.dfsph_step() for _ in range(CAP_STEPS)]
    check_run(stats, o, "caps")
    assert max(s["density_iterations"] for s in stats) == 8 and max(s["divergence_iterations"] for s in stats) == 6
    assert any(s["density_iterations"] < 8 for s in stats) and any(s["divergence_iterations"] < 6 for s in stats)  # and are not all there is


def test_saturated_scene_lies_beyond_the_last_cell():
    """sf 2, particle density 4e6 (h = 0.001), grid_min (-100, -100): every position of the scene, fluid and boundary, maps beyond
    cell 65535 on both axes, and Rust's `as u16` saturates (neighborhood_search.rs:55-56): all particles share cell (65535, 65535).
    That cell is the value prev_morton_pos starts from (neighborhood_search.rs:147-150), so the reference's cell loop never opens a
    cell for them: the cell array is the sentinel alone and par_windows(2) visits no particle (:337) — every list is empty."""
    pos, vel, boundary = cs.scene(cs.SATURATED, SATURATED_N)
    h = cs.properties(cs.SATURATED)["smoothing_length"]
    assert h == np.float32(0.001)
    for xy in (pos, boundary):
        assert (((xy - np.float32(-100.0)) * (np.float32(1.0) / h)) >= np.float32(65536.0)).all()
    o = cs.oracle(cs.SATURATED)
    o.set_boundary(boundary)
    o.set_particles(pos, vel)
    o.update_neighborhood()
    first, cidx = o.cells()
    assert first.tolist() == [SATURATED_N] and cidx.tolist() == [0xFFFFFFFF]
    counts, _, lists = o.neighbors()
    assert (counts == 0).all() and len(lists) == 0 and o.neighbor_flags() == 0
