"""The device away from the reference app's constants: the five parameter sets of tests/constants_scenes.py (h = 0.03, 0.04, 0.01,
0.0025000002, 0.18033393; rest densities 100, 1000, 997, 1, 3.7; oblique gravity; three other grid origins) through every path whose
parity tests so far ran at smoothing factor 2, particle density 10 000, rest density 100, grid_min (-100, -100) only.

sphx_create derives cell_inv, the kernel normalisers, vis_nlap, wc_stiffness, g m / m and fast_walk_ok from the parameter block; the
oracle derives its own copies.  Here the two meet, bit for bit: neighbour lists and densities of the three kernels at three sizes and
both list formats; DFSPH with the adaptive timer and at fixed iterations; WCSPH; the physical viscosity model; xsph_epsilon and the
solver tolerances; cell coordinates that saturate.  The device's sub-steps are also held against the float64 restatement built for the
set, inside the unchanged bound of tests/dfsph_lockstep.py.  Then the features whose references take the constants, at the set `fine`
(shifted grid, oblique gravity, h = 0.01): sampling, per-particle fields, rendering, statistics, save / restore and 2 x 2 tiles.

What each run has to exercise (loops of more than one iteration, warm starts, the iteration caps) is asserted in the oracle alone by
tests/test_constants_reference64.py; the step counts and tolerances used here are that module's."""
import numpy as np
import pytest
import constants_scenes as cs
import test_constants_reference64 as cpu
from dfsph_lockstep import Bounds, check_membership, check_trace, make_plan, membership_of_trace, restatement, run_plan, single_tile
from dfsph_reference64 import brute_force_neighbors
from util import assert_bits_equal, assert_same_neighbors, assert_same_state, step_pair

import yasph2d_amd as y
from yasph2d_amd import _lib
from yasph2d_amd.multi import MultiSolver

pytestmark = pytest.mark.gpu

F = np.float32
KERNELS = [(y.KERNEL_WENDLAND_C2, 0), (y.KERNEL_POLY6, 1), (y.KERNEL_SPIKY, 2)]  # (device, oracle)


def pair(name, n=cs.STEP_N, velocity_scale=0.5, edit=None, **kw):
    """A context and an oracle of the set with the same scene in both.  edit(params): changes to the parameter block."""
    p = cs.params(name, **kw)
    if edit is not None:
        edit(p)
    ctx, o = y.SphxContext(p), cs.oracle(name)
    pos, vel, boundary = cs.scene(name, n, velocity_scale=velocity_scale)
    ctx.set_boundary(boundary)
    o.set_boundary(boundary)
    ctx.upload(pos, vel)
    o.set_particles(pos, vel)
    return ctx, o


def run_pairs(ctx, o, timer, name, steps):
    """`steps` DFSPH steps on both sides: dt in ns, vmax, both iteration counts, both warm-start flags and neighbor_entries of every
    step agree (util.step_pair, with the set's diameter) -> the device's stats."""
    diam = cs.diameter(name)
    stats = [step_pair(ctx, o, timer, diam, f"{name} step {s}") for s in range(steps)]
    assert not (o.neighbor_flags() & 2)
    return stats


def set_span(span):
    def edit(p):
        p.list_span_limit = span
    return edit


# --------------------------------------------------------------------------------------------------------- a. build and densities
@pytest.mark.parametrize("span", [0, y.LISTS_32BIT], ids=["lists16", "lists32"])
@pytest.mark.parametrize("n", cs.CHEAP_N)
@pytest.mark.parametrize("name", cs.SET_IDS)
def test_build_and_densities(name, n, span):
    ctx, o = pair(name, n, edit=set_span(span))
    ctx.update_neighborhood()
    o.update_neighborhood()
    assert o.neighbor_flags() == 0
    lists = ctx.download_neighbors()
    assert_same_neighbors(lists, o.neighbors())
    assert lists[0][:, 1].max() > (20 if name == "wide" else 8)
    if n == 257:  # every particle's list is the brute-force set at the set's h, dynamic entries ascending, then static ones
        s = dict(pos=ctx.download(vel=False, density=False, ids=False)["pos"], boundary=ctx.download_boundary()[0], counts=lists[0], lists=lists[2])
        check_membership(s, float(cs.properties(name)["smoothing_length"]), sample=n, grid_min=cs.SETS[name][4])
    for kd, ko in KERNELS:
        ctx.update_densities(kd)
        o.update_densities(ko)
        assert_bits_equal(ctx.download()["density"], o.densities(), f"{name} n {n} kernel {ko} densities")
    ctx.close()


# ------------------------------------------------------------------------------------------------------------------------ b. c. DFSPH
@pytest.mark.parametrize("name", cs.SET_IDS)
def test_dfsph_adaptive(name):
    ctx, o = pair(name)
    stats = run_pairs(ctx, o, y.TimeManager(), name, cpu.ADAPTIVE_STEPS)
    assert any(s["divergence_iterations"] > 1 for s in stats) and any(s["warmstart_divergence"] for s in stats)
    assert_same_state(ctx, o, name)
    ctx.close()


@pytest.mark.parametrize("span", [0, 64])
@pytest.mark.parametrize("name", cs.SET_IDS)
def test_dfsph_fixed(name, span):
    ctx, o = pair(name, edit=set_span(span), fixed_iterations=(2, 2))
    o.set_fixed_iterations(2, 2)
    ns = cpu.fixed_step_ns(name)
    o.timer_fixed(ns)
    stats = run_pairs(ctx, o, y.TimeManager(fixed_ns=ns), name, cpu.FIXED_STEPS)
    assert all(s["warmstart_density"] and s["warmstart_divergence"] for s in stats[1:])
    assert_same_state(ctx, o, f"{name} span {span}")
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------------------- d. WCSPH
@pytest.mark.parametrize("name", cs.SET_IDS)
def test_wcsph(name):
    """25 WCSPH steps with the adaptive timer at cfl 0.2 (tests/test_gpu_random_scenes.py::test_random_scene_wcsph): dt, vmax, positions,
    velocities and densities equal o.wcsph_step()'s.

    The set `tiny` is a blow-up.  The WCSPH boundary force (wscsph.rs:109-116: Spiky(r) / r^2 with factor 1.0) does not scale with the
    resolution: one spacing (0.001) above the floor at h = 0.0025 it is 1.1e8 m/s^2, and the first step, at the timer's smallest dt
    (41 667 ns), throws the block apart at vmax = 6991.753 m/s, in the oracle and on the device alike.  From step 1 on the particles
    move 0.29 m = 116 cells per step, more than a 64-cell block beyond the covered region: sphx_wcsph_step_begin covers the
    leap-frogged positions before the build when the last step's vmax says so, so that no particle is a stray (kept without
    neighbours for a build: SPHX_FLAG_STRAY_PARTICLES, which include/sphx.h excludes from the parity promise) and the run stays the
    reference's, bit for bit.  Without that cover, vmax of step 1 was 6991.7524 on the device against 6991.719 in the oracle."""
    ctx, o = pair(name)
    timer = y.TimeManager(cfl_factor=0.2)
    o.timer_adaptive(timer.timestep_max_ns, timer.timestep_min_ns, 0.2)
    diam = cs.diameter(name)
    for s in range(cpu.WCSPH_STEPS):
        vmax = ctx.wcsph_step_begin(timer.simulation_step())
        dt_ns = timer.update_simulation_step(diam, vmax)
        ctx.wcsph_step_finish(y.duration_as_secs_f32(dt_ns))
        so = o.wcsph_step()
        assert not ctx.last_flags() & y.FLAG_STRAY_PARTICLES, (name, s)
        assert dt_ns == o.timer_step_ns(), (name, s)
        assert np.float32(vmax) == np.float32(so["vmax"]), (name, s)
    d = ctx.download()
    np.testing.assert_array_equal(d["ids"], o.ids())
    assert_bits_equal(d["pos"], o.positions(), f"{name} positions")
    assert_bits_equal(d["vel"], o.velocities(), f"{name} velocities")
    assert_bits_equal(d["density"], o.densities(), f"{name} densities")
    ctx.close()


# ------------------------------------------------------------------------------------------------------------- e. physical viscosity
def by_id(d):
    order = np.argsort(d["ids"])
    return {k: v[order] for k, v in d.items()}


@pytest.mark.parametrize("name", ["coarse_water", "tiny"])
def test_physical_viscosity_one_step_after_upload_is_exact(name):
    """tests/test_gpu_viscosity.py::test_default_mode_one_step_after_upload_is_exact with the numpy restatement's constants (vis_nlap,
    the mass) derived from the set's parameter block; velocity jumps in 300 particles keep the viscous term far from zero."""
    from tiles_reference import StripLayout, ThreadComm, TiledDFSPH
    from viscosity_reference import PHYSICAL, ViscousOracleTileBackend

    mu = 0.01
    p = cs.params(name, viscosity="physical", fluid_viscosity=mu)
    pos, vel, boundary = cs.scene(name)
    rng = np.random.default_rng(7)
    k = rng.choice(len(vel), 300, replace=False)
    vel[k] += rng.normal(0.0, 50.0 * float(cs.spacing(name)), (len(k), 2)).astype(F)
    diam = cs.diameter(name)
    stats = {}
    for model_mu in (mu, 0.0):
        q = cs.params(name, viscosity="physical", fluid_viscosity=model_mu)
        ctx = y.SphxContext(q)
        ctx.set_boundary(boundary)
        ctx.upload(pos, vel)
        timer = y.TimeManager()
        vmax = ctx.step_begin(timer.simulation_step(), timer.law(diam))
        st = ctx.step_finish(y.duration_as_secs_f32(timer.update_simulation_step(diam, vmax)))
        stats[model_mu] = ((st["density_iterations"], st["divergence_iterations"], timer.simulation_step_ns()),
                           by_id({kk: vv for kk, vv in ctx.download().items() if kk in ("ids", "pos", "vel")}))
        ctx.close()
    assert not np.array_equal(stats[mu][1]["vel"], stats[0.0][1]["vel"]), "the viscous term had no effect"
    t = TiledDFSPH(ViscousOracleTileBackend(PHYSICAL, mu, p, cs.oracle(name)), ThreadComm(ThreadComm.Shared(1), 0), StripLayout(1, [0, 65536]),
                   halo=16, max_avg_density_error=F(p.max_avg_density_error), max_density_iterations=p.max_density_iterations,
                   max_divergence_error=F(p.max_divergence_error), max_divergence_iterations=p.max_divergence_iterations,
                   fluid_density=p.fluid_density, particle_radius=p.particle_radius, h=p.smoothing_length, grid_min=p.grid_min[0])
    assert p.grid_min[0] == p.grid_min[1]  # (TiledDFSPH takes one grid origin for both axes)
    t.setup(pos, vel, None, boundary)
    st = t.step(y.TimeManager())
    ref = by_id(t.download_owned())
    assert stats[mu][0] == (st["density_iterations"], st["divergence_iterations"], st["dt_ns"])
    assert_bits_equal(stats[mu][1]["pos"], ref["pos"], "positions")
    assert_bits_equal(stats[mu][1]["vel"], ref["vel"], "velocities")


# ---------------------------------------------------------------------------------------------------------- f. float64 restatement
@pytest.mark.parametrize("fuse", [False, True], ids=["plain", "fused"])
@pytest.mark.parametrize("name", ["wide", "fine", "odd"])
def test_device_substeps_match_float64_restatement(name, fuse):
    """tests/test_gpu_dfsph_reference64.py::test_device_substeps_match_float64_restatement on the scene and plan of
    tests/test_constants_reference64.py, with the restatement built for the set.  Worst ratio |device - restatement| / bound, plain and
    fused alike: wide 0.112, fine 0.112, odd 0.113 (all in the advection), the oracle's own figures at these sets."""
    from tiles_reference import GpuTileBackend

    b = GpuTileBackend(y.SphxContext(cs.params(name)), own_stream=False)
    pos, vel, boundary = cs.scene(name)
    single_tile(b, pos, vel, boundary)
    trace = run_plan(b, make_plan(3, (3, 2), fuse_predict=fuse, regrid="fused" if fuse else "plain", dt_scale=cpu.dt_scale(name)))
    b.ctx.close()
    bounds = check_trace(trace, restatement(cs.params(name), cs.particle_density(name)), Bounds(), name)
    print(f"\n{name} {'fused' if fuse else 'plain'}: worst ratios\n{bounds.report()}")
    bounds.assert_within()
    membership_of_trace(trace, float(cs.properties(name)["smoothing_length"]), grid_min=cs.SETS[name][4])


# ----------------------------------------------------------------------------------------------------------------- g. solver knobs
@pytest.mark.parametrize("epsilon", [0.0, 0.5])
def test_xsph_epsilon_against_the_oracle(epsilon):
    def edit(p):
        p.xsph_epsilon = epsilon

    ctx, o = pair("coarse_water", edit=edit)
    o.set_xsph_epsilon(epsilon)
    run_pairs(ctx, o, y.TimeManager(), "coarse_water", cpu.KNOB_STEPS)
    assert_same_state(ctx, o, f"xsph_epsilon {epsilon}")
    ctx.close()


def test_tolerances_and_iteration_caps_against_the_oracle():
    """Tolerances no loop meets within 7 / 5 iterations: the counts reach the cap plus one (8 and 6, dfsph.rs:236,391) in the oracle
    and on the device alike, in the same steps; every step's counts (step_pair) and the final state agree bit for bit."""
    tol_d, max_d, tol_v, max_v = cpu.CAP_TOLERANCES

    def edit(p):
        p.max_avg_density_error, p.max_density_iterations, p.max_divergence_error, p.max_divergence_iterations = tol_d, max_d, tol_v, max_v

    ctx, o = pair("coarse_water", velocity_scale=cpu.CAP_VELOCITY_SCALE, edit=edit)
    o.set_tolerances(tol_d, max_d, tol_v, max_v)
    stats = run_pairs(ctx, o, y.TimeManager(), "coarse_water", cpu.CAP_STEPS)
    assert max(s["density_iterations"] for s in stats) == max_d + 1 == 8
    assert max(s["divergence_iterations"] for s in stats) == max_v + 1 == 6
    assert_same_state(ctx, o, "iteration caps")
    ctx.close()


# -------------------------------------------------------------------------------------------------- h. saturated cell coordinates
def rim_aware_brute_force(pos, boundary, h, grid_min, i):
    """dfsph_reference64.brute_force_neighbors under the reference's rule for the rim of the u16 cell domain: a particle in cell 0 or
    65535 of an axis has no neighbours — the box corners `pos.x - 1` / `pos.x + 1` wrap (neighborhood_search.rs:193-194) and, for
    cell (65535, 65535), the cell loop starts from that value and never opens the cell (:147-150)."""
    c = np.clip((pos[i] - np.asarray(grid_min, F)) * (F(1.0) / F(h)), 0.0, 65535.0).astype(np.uint32)
    if ((c == 0) | (c == 65535)).any():
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    return brute_force_neighbors(pos, boundary, h, i)


def test_saturated_cell_coordinates():
    """sf 2, particle density 4e6 (h = 0.001), default grid_min, 300 particles at the scene's origin: every position maps beyond cell
    65535 on both axes and `as u16` saturates, so all particles share cell (65535, 65535).  That is a rim cell: by the reference's own
    arithmetic no particle there has a neighbour (tests/test_constants_reference64.py::test_saturated_scene_lies_beyond_the_last_cell),
    although the plain distance rule finds 12 for most of them.  Lists equal the oracle's and the rim-aware brute force; densities of
    the three kernels are bit-equal (the self term, clamped to rho0); no stepping."""
    ctx, o = pair(cs.SATURATED, cpu.SATURATED_N)
    ctx.update_neighborhood()
    o.update_neighborhood()
    lists = ctx.download_neighbors()
    assert_same_neighbors(lists, o.neighbors())
    counts, start, entries = lists
    pos, boundary = ctx.download(vel=False, density=False, ids=False)["pos"], ctx.download_boundary()[0]
    h = cs.properties(cs.SATURATED)["smoothing_length"]
    plain = 0
    for i in range(len(pos)):
        dyn, stat = rim_aware_brute_force(pos, boundary, h, cs.SATURATED[4], i)
        nd, nt = int(counts[i, 0]), int(counts[i, 1])
        e = entries[int(start[i]):int(start[i]) + nt].astype(np.int64)
        assert np.array_equal(e[:nd], dyn) and np.array_equal(e[nd:], stat), i
        plain += len(brute_force_neighbors(pos, boundary, h, i)[0])
    assert plain > 8 * len(pos)  # (the distance rule alone would have filled the lists)
    for kd, ko in KERNELS:
        ctx.update_densities(kd)
        o.update_densities(ko)
        assert_bits_equal(ctx.download()["density"], o.densities(), f"saturated, kernel {ko}")
    ctx.close()


# =========================================================================================== features at the set `fine`
FINE = "fine"


def device_steps(ctx, timer, k, diam):
    out = []
    for _ in range(k):
        vmax = ctx.step_begin(timer.simulation_step(), timer.law(diam))
        dt_ns = timer.update_simulation_step(diam, vmax)
        out.append((ctx.step_finish(y.duration_as_secs_f32(dt_ns)), dt_ns))
    return out


def fine_context(steps=cpu.FEATURE_STEPS, **kw):
    ctx = y.SphxContext(cs.params(FINE, **kw))
    pos, vel, boundary = cs.scene(FINE)
    ctx.set_boundary(boundary)
    ctx.upload(pos, vel)
    timer = y.TimeManager()
    device_steps(ctx, timer, steps, cs.diameter(FINE))
    return ctx, timer


@pytest.fixture(scope="module")
def fine10():
    """The 1500-particle scene of the set `fine` after 10 adaptive steps: shared, never stepped again."""
    ctx, timer = fine_context()
    yield ctx
    ctx.close()


def test_sample_points_at_fine(fine10):
    """sample_reference.sample32 with the set's constants gives the exact contract bits on a seeded cloud of 500 points: in the fluid,
    around it, and left of / below grid_min (cell coordinate clamped to 0)."""
    import sample_reference as sr
    import test_gpu_sample as ts

    ctx = fine10
    K, st = ts.consts_of(ctx), ts.state_of(ctx)
    assert K.h == F(0.01) and tuple(K.gmin) == (F(-3.0), F(-7.5))
    rng = np.random.default_rng(41)
    lo, hi = st["pos"].min(0), st["pos"].max(0)
    span = hi - lo
    pts = np.concatenate([
        st["pos"][rng.choice(len(st["pos"]), 100, replace=False)] + rng.normal(0, 0.003, (100, 2)),   # in the fluid
        rng.uniform(lo - 0.5 * span, hi + 0.5 * span, (300, 2)),                                       # in and around it
        st["boundary"][rng.choice(len(st["boundary"]), 40, replace=False)] + rng.normal(0, 0.003, (40, 2)),
        np.stack([rng.uniform(-3.5, -3.0001, 30), rng.uniform(lo[1], hi[1], 30)], -1),                # left of grid_min
        np.stack([rng.uniform(lo[0], hi[0], 30), rng.uniform(-8.0, -7.5001, 30)], -1)]).astype(F)      # below grid_min
    assert len(pts) == 500 and (pts[:, 0] < F(-3.0)).sum() == 30
    for kind in ts.KINDS:
        ref = sr.sample32(K, st, pts, kind)
        assert (ref["count"][:100] > 0).all() and (ref["count"][100:400] == 0).any() and not ref["count"][440:].any()
        ts.assert_bits(ctx.sample(pts, kind), ref, "fine, kind %d" % kind)


def test_particle_fields_at_fine(fine10):
    import fields_reference as fr
    import test_gpu_fields as tf

    ctx = fine10
    st, counts, lists = tf.state_of(ctx)
    ref = fr.fields32(tf.consts_of(ctx), st, counts, lists)
    assert all(np.abs(ref[f]).max() > 0 for f in tf.NAMES)
    tf.assert_bits(ctx.fields(), ref, "fine, host path")
    tf.assert_bits(tf.device_path(ctx), ref, "fine, device-pointer path")


def test_render_at_fine(fine10):
    """render_reference.render32 draws the discs at the set's particle_radius (0.0025): same owners and RGBA on a 160 x 120 frame fitted
    to the scene."""
    import render_reference as rr
    import test_gpu_render as tr

    ctx = fine10
    st = tr.state_of(ctx)
    assert tr.radius_of(ctx) == cs.properties(FINE)["particle_radius"] == F(0.0025)
    xy = np.concatenate([st["pos"], st["boundary"]])
    lo, hi = xy.min(0), xy.max(0)
    rect = (float(lo[0]) - 0.01, float(lo[1]) - 0.01, float(hi[0] - lo[0]) + 0.02, float(hi[1] - lo[1]) + 0.02)
    view = rr.fit(160, 120, rect)
    fitted = y.render_fit(160, 120, rect)
    assert (F(fitted.pixel_per_world_unit), tuple(F(c) for c in fitted.center)) == (view.pixel_per_world_unit, view.center)
    ref = tr.check_view(ctx, st, view, "fine 160x120", singles=True)
    fluid = ref["owner"] < rr.BOUNDARY
    assert fluid.mean() >= 0.02 and (ref["owner"] == rr.BOUNDARY).any() and (ref["owner"] == rr.NONE).mean() >= 0.02
    # another radius draws another picture: the set's radius is what the reference was given
    other = rr.render32(st, view, F(0.005))
    assert not np.array_equal(other["owner"], ref["owner"])


def test_fluid_stats_at_fine(fine10):
    import test_gpu_stats as tstats

    ctx = fine10
    d = ctx.download()
    lo, hi = d["pos"].min(0), d["pos"].max(0)
    mid = 0.5 * (lo + hi)
    rects = [(float(lo[0]), float(lo[1]), float(mid[0]), float(mid[1])), (float(mid[0]), float(lo[1]), tstats.INF, float(hi[1])),
             (-3.5, -8.0, -3.0, -7.5), tstats.EVERYTHING]
    got = ctx.stats(rects)
    tstats.check_all(got, d, rects, True, "fine")
    c = got["count"].tolist()
    assert c[0] == cs.STEP_N == c[4] and 0 < c[1] < cs.STEP_N and 0 < c[2] < cs.STEP_N and c[3] == 0


def test_state_save_and_restore_at_fine():
    """A blob saved after 10 steps, loaded into a fresh context of the same parameter block, then 5 steps: bit-equal to the
    uninterrupted run.  A context made with default_params() refuses the blob and stays what it was."""
    import test_gpu_state as tstate
    from util import lattice_scene

    diam = cs.diameter(FINE)
    a, ta = fine_context()
    blob = a.save_state()
    b, tb = y.SphxContext(cs.params(FINE)), tstate.timer_like(ta)
    b.load_state(blob)
    assert b.state_digest() == a.state_digest()
    sa, sb = device_steps(a, ta, 5, diam), device_steps(b, tb, 5, diam)
    assert sa == sb
    tstate.assert_same_arrays(tstate.full_state(a), tstate.full_state(b), "5 steps after the restore")
    # the reference app's parameter block: refused, untouched
    pos, boundary = lattice_scene(257, 37)
    c, twin = y.SphxContext(y.default_params()), y.SphxContext(y.default_params())
    tc, tt = y.TimeManager(), y.TimeManager()
    for ctx in (c, twin):
        ctx.set_boundary(boundary)
        ctx.upload(pos)
    assert device_steps(c, tc, 2, F(0.01)) == device_steps(twin, tt, 2, F(0.01))
    before = c.state_digest()
    tstate.refused(_lib.ERR_INVALID_ARGUMENT, c.load_state, blob)
    assert c.state_digest() == before == twin.state_digest()
    assert device_steps(c, tc, 2, F(0.01)) == device_steps(twin, tt, 2, F(0.01))
    tstate.assert_same_arrays(tstate.full_state(c), tstate.full_state(twin), "after the refused load")
    for ctx in (a, b, c, twin):
        ctx.close()


def test_tiles_at_fine(fine10):
    """sphx_multi on 2 x 2 tiles of one device in tiling-invariant mode at fixed (2, 2), 8 steps from the shared state, against the
    single context in the same mode, matched by id (the comparison of tests/test_gpu_multi.py); then sphx_multi_sample_points and
    sphx_multi_particle_fields against the single context's answers.  The cuts are cell indices relative to grid_min (-3, -7.5) at
    h = 0.01: the only place where tile cuts and ghost bands meet another cell grid."""
    import test_gpu_sample as ts
    from tiles_reference import cell_coord

    d0 = fine10.download()
    boundary = fine10.download_boundary()[0]
    order = np.argsort(d0["ids"])
    pos, vel = d0["pos"][order], d0["vel"][order]
    n, steps, diam = len(pos), 8, cs.diameter(FINE)
    h, gm = float(cs.properties(FINE)["smoothing_length"]), cs.SETS[FINE][4]
    ctx = y.SphxContext(cs.params(FINE, fixed_iterations=(2, 2)))
    ctx.set_tiling_invariant(True)
    ctx.set_boundary(boundary)
    ctx.upload(pos, vel)
    timer = y.TimeManager()
    stats = device_steps(ctx, timer, steps, diam)
    assert sum(st["warmstart_density"] + st["warmstart_divergence"] for st, _ in stats) >= 2 * (steps - 1)
    s = ctx.download()
    ref = by_id({k: s[k] for k in ("ids", "pos", "vel")})
    cx, cy = cell_coord(pos, 0, gm[0], h=h), cell_coord(pos, 1, gm[1], h=h)
    assert 300 < cx.min() and cx.max() < 500 and 700 < cy.min() and cy.max() < 900  # (cells of the shifted grid, not of the default one)
    xcuts = [0, int(np.sort(cx)[int(0.4 * n)]), 65536]
    ycuts = []
    for ix in range(2):
        col = cy[(cx >= xcuts[ix]) & (cx < xcuts[ix + 1])]
        ycuts.append([0, int(np.sort(col)[len(col) // 2]), 65536])
    m = MultiSolver(cs.params(FINE, fixed_iterations=(2, 2)), devices=[0, 0, 0, 0], halo=8, rebalance_every=4)
    m.set_tiling_invariant(True)
    m.set_grid(xcuts, np.array(ycuts, np.uint32))
    m.set_boundary(boundary)
    m.upload(pos, vel)
    t2 = y.TimeManager()
    for _ in range(steps):
        m.step(t2, diam)
    a = by_id({k: v for k, v in m.download().items() if k in ("ids", "pos", "vel")})
    np.testing.assert_array_equal(a["ids"], np.arange(n, dtype=np.uint32))
    assert_bits_equal(a["pos"], ref["pos"], "positions, 2 x 2 tiles at fine")
    assert_bits_equal(a["vel"], ref["vel"], "velocities, 2 x 2 tiles at fine")
    assert t2.simulation_step_ns() == timer.simulation_step_ns()
    info = m.info()
    assert info["owned_local"] == n and info["build_particles"] > n  # ghosts exist
    # the queries of a tiled run against the single context's
    rng = np.random.default_rng(43)
    lo, hi = ref["pos"].min(0), ref["pos"].max(0)
    pts = np.concatenate([ref["pos"][::5] + rng.normal(0, 0.003, ref["pos"][::5].shape), rng.uniform(lo - 0.05, hi + 0.05, (200, 2)),
                          np.array([[-3.2, 0.2], [0.4, -7.7], [-50.0, -50.0]])]).astype(F)
    for kind in ts.KINDS:
        ts.assert_bits(m.sample(pts, kind), ctx.sample(pts, kind), "2 x 2 tiles at fine, kind %d" % kind)
    got = m.fields(by_id=True)
    assert np.array_equal(got["ids"], np.arange(n, dtype=np.uint32))
    f = ctx.fields()
    o2 = np.argsort(s["ids"], kind="stable")
    for name in f:
        assert np.array_equal(np.ascontiguousarray(got[name]).view(np.uint32), np.ascontiguousarray(f[name][o2]).view(np.uint32)), name
    m.close()
    ctx.close()
