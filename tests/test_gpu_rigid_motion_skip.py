"""The rigid form of the non-pressure pass ("Rigid motion"): while every fluid velocity carries the bits of
vel[0] the XSPH / viscosity sum adds exact zeros, and the run-ahead pass stores K.a instead of walking the lists.

Every scene runs four ways in lock step — SPHX_RIGID_SKIP=1 ("on": under the hint), =force with SPHX_QUIET_TAKEOVER=force ("forced":
every run-ahead pass behind a thin divergence correction is queued in the rigid form, whatever it will find), =0 ("off": the launches
from before) and the CPU oracle — and positions, velocities, densities, the acceleration array the run-ahead pass left, vmax, dt in
nanoseconds, the iteration counts and the step flags must agree bit for bit in every step.  (The oracle has no accessor for the
accelerations: the three contexts are compared with one another, and the oracle checks what comes of them, vmax and the next step's
velocities.  It has no physical viscosity model and no sphx_append / sphx_remove either: those scenes compare the three contexts.)

sphx_debug_rigid_counts -> (passes queued in the rigid form, those that found no mark and stored K.a, those that found a mark and ran
the full body).  What they must read, for a scene whose loops take one iteration each:
    forced: the divergence correction is thin from step 0, so every step's run-ahead pass is rigid: one launch per step;
    on:     the correction is thin from step 1 (the quiet hint), the pass behind it is judged (k_rigid_judge), sphx_step_begin reads
            the verdict in step 2, and from the end of step 2 the pass is rigid while no judged pass has found a mark.

-0 against +0 needs an acceleration whose a.x dt is -0: the velocity prediction in front of the gather computes v + a dt, and with
a.x = +0 it turns -0 + (+0) into +0 before the first gather compares anything (with a.x = -0 the rigid form is never queued).  A
gravity x of -3e-43 gives it: K.a.x stays a non-zero denormal, which the host's test accepts, a.x dt underflows to -0, and
-0 + (-0) = -0 for the odd particle while the block keeps +0 + (-0) = +0.  Both cases have a test.

One of the issue's scenes cannot reach a gather through the interface: with a NaN or infinite velocity the step's maximum velocity
is not finite and sphx_step_begin fails (as the reference panics) before any gather has run.  Its test asserts that course.
"""
import numpy as np
import pytest
from test_gpu_quiet_scene import patch_scene
from util import assert_bits_equal, lattice_scene

import yasph2d_amd as y
from oracle.oracle import Oracle

pytestmark = pytest.mark.gpu

DIAM = np.float32(0.01)
STAT_KEYS = ("density_iterations", "divergence_iterations", "warmstart_density", "warmstart_divergence", "neighbor_entries", "flags")
ENVS = {
    "on": {"SPHX_RIGID_SKIP": "1", "SPHX_THIN_GRID": "5"},
    "forced": {"SPHX_RIGID_SKIP": "force", "SPHX_QUIET_TAKEOVER": "force", "SPHX_THIN_GRID": "3"},
    "off": {"SPHX_RIGID_SKIP": "0"},
}
N = 20000  # 79 blocks of 256 (a grid of 80): five resp. three workgroups loop over them, ragged


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def make_ctx(monkeypatch, env, pos, vel, boundary, fixed, gravity, viscosity):
    """The switches are read once, in sphx_create.  SPHX_ZERO_SKIP=1: the flags (and with them the thin corrections) at this size."""
    env = dict(env, SPHX_ZERO_SKIP="1")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    p = y.default_params(fixed_iterations=fixed, viscosity=viscosity)
    p.gravity[0], p.gravity[1] = gravity
    ctx = y.SphxContext(p)
    for k in env:
        monkeypatch.delenv(k)
    if boundary is not None:
        ctx.set_boundary(boundary)
    ctx.upload(pos, vel)
    return ctx


class Quad:
    def __init__(self, monkeypatch, pos, vel=None, boundary=None, fixed=(0, 0), gravity=(0.0, -9.81), viscosity="xsph", oracle=True):
        self.ctx = {k: make_ctx(monkeypatch, e, pos, vel, boundary, fixed, gravity, viscosity) for k, e in ENVS.items()}
        self.timer = {k: y.TimeManager() for k in ENVS}
        self.o = None
        if oracle:
            self.o = Oracle(gravity=gravity)
            self.o.set_fixed_iterations(*fixed)
            if boundary is not None:
                self.o.set_boundary(boundary)
            self.o.set_particles(pos, vel)
        self.counts = {k: [] for k in ENVS}  # per step: the step's (launches, exits, marked)
        self.stats = []

    def step(self, what=""):
        so = self.o.dfsph_step() if self.o else None
        seen = {}
        for k, ctx in self.ctx.items():
            timer = self.timer[k]
            c0 = ctx.rigid_counts()
            vmax = ctx.step_begin(timer.simulation_step(), timer.law(DIAM))
            dt_ns = timer.update_simulation_step(DIAM, vmax)
            st = ctx.step_finish(y.duration_as_secs_f32(dt_ns))
            self.counts[k].append(tuple(b - a for a, b in zip(c0, ctx.rigid_counts())))
            seen[k] = (np.float32(vmax).view(np.uint32), dt_ns) + tuple(st[s] for s in STAT_KEYS)
            if so:
                assert dt_ns == self.o.timer_step_ns(), (what, k)
                assert np.float32(vmax) == np.float32(so["vmax"]), (what, k, vmax, so["vmax"])
                for s in STAT_KEYS[:-1]:
                    assert st[s] == so[s], (what, k, s, st[s], so[s])
        assert seen["on"] == seen["off"] == seen["forced"], (what, seen)
        print(what, {k: v[-1] for k, v in self.counts.items()}, "iterations", seen["off"][2:4])
        self.stats.append(seen["off"])
        self.compare(what)
        return seen["off"]

    def compare(self, what=""):
        ref = self.ctx["off"].download()
        acc = self.ctx["off"].download_accel()
        for k in ("on", "forced"):
            d = self.ctx[k].download()
            np.testing.assert_array_equal(d["ids"], ref["ids"], f"{what} {k} ids")
            for f in ("pos", "vel", "density"):
                assert np.array_equal(bits(d[f]), bits(ref[f])), f"{what} {k} {f}"
            assert np.array_equal(bits(self.ctx[k].download_accel()), bits(acc)), f"{what} {k} accelerations"
        if self.o:
            np.testing.assert_array_equal(ref["ids"], self.o.ids(), what + " ids")
            assert_bits_equal(ref["pos"], self.o.positions(), what + " positions")
            assert_bits_equal(ref["vel"], self.o.velocities(), what + " velocities")
            assert_bits_equal(ref["density"], self.o.densities(), what + " densities")
        assert self.ctx["off"].rigid_counts() == (0, 0, 0), "SPHX_RIGID_SKIP=0 queues the launches from before"
        return acc

    def run(self, steps, what=""):
        return [self.step(f"{what} step {s}") for s in range(steps)]


def block(n=N, v=(0.0, 0.0)):
    """n lattice particles (8 neighbours inside h: densities below rho0, every factor zero), no boundary in reach: free fall"""
    pos, _ = lattice_scene(n, 1)
    return pos, np.tile(np.asarray(v, np.float32), (n, 1))


def sorted_ids(pos):
    """original index of the particle at every sorted slot (the oracle's Morton order is the device's)"""
    o = Oracle()
    o.set_particles(pos)
    o.update_neighborhood()
    return o.ids()


def uniform(vel):
    return bool((bits(vel) == bits(vel)[0]).all())


FREE_ON = [(0, 0, 0), (0, 0, 0)]  # "on": no thin correction in step 0, a judged full pass behind step 1


def test_lattice_block_in_free_fall(monkeypatch):
    """All rigid exits: the forced context's pass is a fill from the one that serves the second step on, the hinted one's from the end
    of step 2.  The stored accelerations are K.a, the velocities stay one bit pattern (checked on the oracle's)."""
    pos, vel = block(v=(0.25, 0.0))
    q = Quad(monkeypatch, pos, vel)
    for s in range(6):
        st = q.step(f"step {s}")
        assert st[2:4] == (1, 1)
        assert uniform(q.o.velocities()), "rigid translation"
        acc = q.ctx["on"].download_accel()
        assert uniform(acc) and acc[0, 0] == 0 and not np.signbit(acc[0, 0]) and abs(acc[0, 1] + 9.81) < 1e-5, acc[0]
    assert q.counts["forced"] == [(1, 1, 0)] * 6, q.counts
    assert q.counts["on"] == FREE_ON + [(1, 1, 0)] * 4, q.counts


@pytest.mark.parametrize("where", ["first wavefront", "last wavefront", "alone"])
def test_one_particle_with_another_velocity(monkeypatch, where):
    """The block plus one particle whose velocity differs in x: in the first wavefront of the sorted order, in the last, or alone, ten
    smoothing lengths away (no neighbour at all).  Every forced pass finds the gather's mark and runs the full body over its blocks;
    the hinted context never queues the rigid form."""
    pos, vel = block()
    ids = sorted_ids(pos)
    if where == "alone":
        pos = np.concatenate([pos, pos[:1] - np.float32(0.2)]).astype(np.float32)
        vel = np.concatenate([vel, vel[:1]])
        odd = len(pos) - 1
    else:
        odd = int(ids[5] if where == "first wavefront" else ids[len(ids) - 3])
    vel[odd, 0] = np.float32(1e-3)
    q = Quad(monkeypatch, pos, vel)
    q.run(4, where)
    sid = q.o.ids()
    slot = int(np.nonzero(sid == odd)[0][0])
    if where == "first wavefront":
        assert slot < 64
    if where == "last wavefront":
        assert slot >= (len(pos) - 1) // 64 * 64
    if where == "alone":
        counts, _, _ = q.o.neighbors()
        assert counts[slot, 1] == 0
    assert not uniform(q.o.velocities())
    assert q.counts["on"] == [(0, 0, 0)] * 4, q.counts
    assert all(c == (1, 0, 1) for c in q.counts["forced"]), q.counts


def test_negative_zero_against_plus_zero_is_marked(monkeypatch):
    """Same speed, other bits: one particle's x velocity is -0 where the block's is +0, under a gravity x of -3e-43 (module docstring).
    On the oracle exactly one particle still carries -0 in x after every step, and the velocities compare equal as numbers.  The
    gather's comparison is one of bits: every forced pass finds its mark and runs the full body, the hinted context's judged pass
    finds it too and the rigid form is never queued.  (A comparison of floats in the gather would read rigid exits here.)"""
    gravity = (-3e-43, -9.81)
    pos, vel = block()
    odd = int(sorted_ids(pos)[N // 2 + 7])
    vel[odd, 0] = np.float32(-0.0)
    q = Quad(monkeypatch, pos, vel, gravity=gravity)
    for s in range(4):
        st = q.step(f"step {s}")
        assert st[2:4] == (1, 1)
        v = q.o.velocities()
        assert np.count_nonzero(np.signbit(v[:, 0])) == 1 and int(q.o.ids()[np.signbit(v[:, 0])][0]) == odd, "one -0 survives"
        assert (v == v[0]).all() and not uniform(v), "equal as numbers, not as bits"
        acc = q.ctx["off"].download_accel()
        assert uniform(acc) and acc[0, 0] < 0 and abs(acc[0, 0]) < 1e-38, "K.a.x is a non-zero denormal"
    assert q.counts["on"] == [(0, 0, 0)] * 4, q.counts
    assert q.counts["forced"] == [(1, 0, 1)] * 4, q.counts


def test_negative_zero_is_gone_after_the_prediction_when_a_x_is_plus_zero(monkeypatch):
    """The same particle under the default gravity (a.x = +0): the prediction of step 0 computes -0 + (+0) dt = +0 in front of the
    first gather, the oracle's velocities are one bit pattern after step 0, and the passes are the free fall's."""
    pos, vel = block()
    vel[len(pos) // 2, 0] = np.float32(-0.0)
    assert not uniform(vel)
    q = Quad(monkeypatch, pos, vel)
    q.run(4)
    assert uniform(q.o.velocities()) and not np.signbit(q.o.velocities()[:, 0]).any()
    assert q.counts["forced"] == [(1, 1, 0)] * 4 and q.counts["on"] == FREE_ON + [(1, 1, 0)] * 2, q.counts


@pytest.mark.parametrize("bad", ["nan", "inf"])
def test_non_finite_velocity_takes_the_same_course(monkeypatch, bad):
    """One NaN or infinite velocity component.  The step does not survive it — SPHX_ERR_NONFINITE from sphx_step_begin, before any
    gather — and whatever it left is the same bits in all three contexts; no rigid pass was queued."""
    pos, vel = block()
    vel[len(pos) // 2, 1] = np.float32(bad)
    out = []
    for env in ENVS.values():
        ctx = make_ctx(monkeypatch, env, pos, vel, None, (0, 0), (0.0, -9.81), "xsph")
        timer = y.TimeManager()
        with pytest.raises(y.SphxError) as e:
            ctx.step_begin(timer.simulation_step(), timer.law(DIAM))
        assert e.value.code == y._lib.ERR_NONFINITE
        assert ctx.rigid_counts() == (0, 0, 0)
        d = ctx.download()
        out.append((d["pos"], d["vel"], d["density"], ctx.download_accel()))
    for a, b, c in zip(*out):
        assert np.array_equal(bits(a), bits(b)) and np.array_equal(bits(a), bits(c))


def test_quiet_end(monkeypatch):
    """The patch of tests/test_gpu_quiet_scene.py falls towards a boundary row until, in step 2, the density loop has factors: its thin
    correction walks and changes velocities in front of the gather, whose marks send the rigid pass queued behind that step through
    the full body.  The verdict clears the hint: the hinted context queues no rigid pass afterwards."""
    pos, boundary = patch_scene(N)
    q = Quad(monkeypatch, pos, boundary=boundary)
    marked_at = None
    for s in range(5):
        q.step(f"step {s}")
        if marked_at is None and np.any(q.o.kappa() != 0):
            marked_at = s
            assert not uniform(q.o.velocities()), "the correction changed some velocities"
    assert marked_at == 2, marked_at
    assert q.counts["on"] == FREE_ON + [(1, 0, 1), (0, 0, 0), (0, 0, 0)], q.counts
    assert q.counts["forced"][:2] == [(1, 1, 0)] * 2 and q.counts["forced"][2] == (1, 0, 1), q.counts
    assert all(c[1] == 0 for c in q.counts["forced"][2:]), q.counts


def test_gravity_with_a_negative_zero_component(monkeypatch):
    """K.a = (-0, g): -0 + (+0) is +0, not K.a — the rigid form is never queued, forced or not."""
    pos, vel = block()
    q = Quad(monkeypatch, pos, vel, gravity=(-0.0, -9.81))
    q.run(4)
    acc = q.ctx["off"].download_accel()
    assert not np.signbit(acc[:, 0]).any(), "the walk's sum turns -0 into +0 wherever a particle has a dynamic neighbour"
    assert q.counts["on"] == q.counts["forced"] == [(0, 0, 0)] * 4, q.counts


def test_physical_viscosity_model(monkeypatch):
    """k_nonpressure_rigid<PHYSICAL>: the free fall's exits, and the full body behind a mark (one particle with another velocity)."""
    pos, vel = block(v=(0.0, -0.125))
    q = Quad(monkeypatch, pos, vel, viscosity="physical", oracle=False)
    q.run(4, "physical, rigid")
    assert q.counts["forced"] == [(1, 1, 0)] * 4 and q.counts["on"] == FREE_ON + [(1, 1, 0)] * 2, q.counts
    vel[int(sorted_ids(pos)[N // 2]), 0] = np.float32(1e-3)
    q = Quad(monkeypatch, pos, vel, viscosity="physical", oracle=False)
    q.run(3, "physical, mixed")
    assert q.counts["on"] == [(0, 0, 0)] * 3 and q.counts["forced"] == [(1, 0, 1)] * 3, q.counts
    acc = q.ctx["on"].download_accel()
    assert (acc[:, 0] != 0).any(), "the viscous term is at work"


def test_second_divergence_iteration_voids_the_record(monkeypatch):
    """The issue's "a step with a divergence warm start between two rigid steps" cannot be built: the iteration counts are creation
    parameters (sphx_params.fixed_*_iterations; nothing sets them mid-run), and an adaptive loop that takes a second iteration has
    corrected velocities, so no rigid step follows it.  What can be shown is that the warm start and the second correction void the
    record, step after step.
    fixed_iterations = (1, 2): every divergence loop has a warm start in front of it (from step 1 on) and a second correction in the
    old form behind its first — both can write velocities behind the gather, so no run-ahead pass is judged, forced or not.  One
    exception, and it changes nothing: step 0 predicts one iteration, so the forced context queues its (rigid) pass behind the first,
    thin correction; the loop then needs its second iteration, and the pass is discarded and run again in full by sphx_step_begin."""
    pos, vel = block()
    q = Quad(monkeypatch, pos, vel, fixed=(1, 2))
    st = q.run(4)
    assert st[-1][4:6] == (0, 1), "warm start in front of the divergence loop"
    assert q.counts["on"] == [(0, 0, 0)] * 4 and q.counts["forced"] == [(1, 1, 0)] + [(0, 0, 0)] * 3, q.counts


@pytest.mark.parametrize("event", ["append", "remove", "upload", "state_load"])
def test_edits_and_loads_void_the_record_and_the_hint(monkeypatch, event):
    """Four rigid steps, the event, four more.  The pass that ran ahead of the event is not adopted (the next step runs the full pass
    in sphx_step_begin), the hint is gone — the hinted context needs a thin step and a judged step again — and the bits stay the
    off context's all along.  The oracle follows the upload (a fresh one, from the downloaded state, as the contexts start afresh) and
    the load (it just goes on); it has no sphx_append / sphx_remove: there the three contexts are compared."""
    pos, vel = block(v=(0.0, -0.5))
    q = Quad(monkeypatch, pos, vel, oracle=event in ("upload", "state_load"))
    q.run(4, "before")
    assert q.counts["on"][-1] == (1, 1, 0)
    for k, ctx in q.ctx.items():
        if event == "append":
            d = ctx.download()
            ctx.append(pos[:300] - np.float32([0.0, 0.3]), np.tile(d["vel"][:1], (300, 1)))  # (a strip below the block, at its velocity)
        elif event == "remove":
            assert ctx.remove((0.0, 0.0, 0.55, 10.0)) > 0
        elif event == "upload":
            d = ctx.download()
            ctx.clear_cached()
            ctx.upload(d["pos"], d["vel"])
            q.timer[k] = y.TimeManager()
        else:
            ctx.load_state(ctx.save_state())
    if event == "upload":
        q.o = Oracle()
        q.o.set_particles(d["pos"], d["vel"])
    for k in q.counts:
        q.counts[k].clear()
    q.run(4, "after " + event)
    assert q.counts["on"] == FREE_ON + [(1, 1, 0)] * 2, q.counts
    assert q.counts["forced"] == [(1, 1, 0)] * 4, q.counts
