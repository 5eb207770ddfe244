"""The rigid form of the first density producer ("Rigid motion"): a rigid non-pressure pass that finds no mark
leaves accel[] unwritten, and the velocity prediction + compute_density_error behind it (k_compute_error_rigid) reads K.a from its
arguments; a workgroup none of whose particles has a static neighbour leaves without a list word or a neighbour's record.

Every scene runs in lock step in five device contexts and, where it has the scene's model, the CPU oracle:
    on      SPHX_RIGID_SKIP=1: the forms under their hints
    forced  SPHX_RIGID_SKIP=force, SPHX_QUIET_TAKEOVER=force: every run-ahead pass behind a thin divergence correction is rigid, the
            density loop's first producer is the take-over form from step 0 — so every step from the second on queues the new form
    accel   forced, with SPHX_RIGID_PREDICT=accel: K.a from the arguments, no fluid-only exit
    fill    forced, with SPHX_RIGID_PREDICT=0: the rigid pass stores K.a itself, no record, the launches from before
    off     SPHX_RIGID_SKIP=0
Positions, velocities, densities, kappa, the acceleration array (sphx_debug_download_accel: it materialises what the pass left out,
and must not change the course), the cell arrays of the step's build (the count behind them is the speculative one of the step
before), vmax bits, dt in nanoseconds, the iteration counts and the flags agree bit for bit in every step.

sphx_debug_rigid_predict_counts -> (launches of the new form, workgroups that left through the exit, workgroups that walked with
K.a, launches that found no verdict), per step below.  SPHX_ZERO_SKIP_COUNT=1 in every context.
"""
import numpy as np
import pytest
from test_gpu_quiet_scene import patch_scene
from test_gpu_rigid_motion_skip import DIAM, STAT_KEYS, bits, block, sorted_ids, uniform

import yasph2d_amd as y
from oracle.oracle import Oracle
from util import assert_bits_equal

pytestmark = pytest.mark.gpu

FORCED = {"SPHX_RIGID_SKIP": "force", "SPHX_QUIET_TAKEOVER": "force", "SPHX_THIN_GRID": "3"}
ENVS = {
    "on": {"SPHX_RIGID_SKIP": "1", "SPHX_THIN_GRID": "5"},
    "forced": FORCED,
    "accel": dict(FORCED, SPHX_RIGID_PREDICT="accel"),
    "fill": dict(FORCED, SPHX_RIGID_PREDICT="0"),
    "off": {"SPHX_RIGID_SKIP": "0"},
}
N = 20000  # 79 blocks of 256
ZERO = (0, 0, 0, 0)


def blocks_of(n):
    return (n + 255) // 256


def make_ctx(monkeypatch, env, pos, vel, boundary, fixed, gravity, viscosity, span):
    env = dict(env, SPHX_ZERO_SKIP="1", SPHX_ZERO_SKIP_COUNT="1")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    p = y.default_params(fixed_iterations=fixed, viscosity=viscosity)
    p.gravity[0], p.gravity[1] = gravity
    p.list_span_limit = span
    ctx = y.SphxContext(p)
    for k in env:
        monkeypatch.delenv(k)
    if boundary is not None:
        ctx.set_boundary(boundary)
    ctx.upload(pos, vel)
    return ctx


class Quint:
    def __init__(self, monkeypatch, pos, vel=None, boundary=None, fixed=(0, 0), gravity=(0.0, -9.81), viscosity="xsph", oracle=True, span=0,
                 names=tuple(ENVS)):
        self.ctx = {k: make_ctx(monkeypatch, ENVS[k], pos, vel, boundary, fixed, gravity, viscosity, span) for k in names}
        self.timer = {k: y.TimeManager() for k in names}
        self.o = None
        if oracle:
            self.o = Oracle(gravity=gravity)
            self.o.set_fixed_iterations(*fixed)
            if boundary is not None:
                self.o.set_boundary(boundary)
            self.o.set_particles(pos, vel)
        self.counts = {k: [] for k in names}  # per step: the step's rigid_predict_counts
        self.rigid = {k: [] for k in names}   # ... and rigid_counts

    def step_one(self, k):
        ctx, timer = self.ctx[k], self.timer[k]
        c0, r0 = ctx.rigid_predict_counts(), ctx.rigid_counts()
        vmax = ctx.step_begin(timer.simulation_step(), timer.law(DIAM))
        dt_ns = timer.update_simulation_step(DIAM, vmax)
        st = ctx.step_finish(y.duration_as_secs_f32(dt_ns))
        self.counts[k].append(tuple(b - a for a, b in zip(c0, ctx.rigid_predict_counts())))
        self.rigid[k].append(tuple(b - a for a, b in zip(r0, ctx.rigid_counts())))
        return (int(np.float32(vmax).view(np.uint32)), dt_ns) + tuple(st[s] for s in STAT_KEYS)

    def step(self, what="", download_accel=True):
        so = self.o.dfsph_step() if self.o else None
        seen = {k: self.step_one(k) for k in self.ctx}
        if so:
            assert seen["off"][1] == self.o.timer_step_ns(), what
            assert np.uint32(seen["off"][0]).view(np.float32) == np.float32(so["vmax"]), what
            for j, s in enumerate(STAT_KEYS[:-1]):
                assert seen["off"][2 + j] == so[s], (what, s)
        assert all(v == seen["off"] for v in seen.values()), (what, seen)
        print(what, {k: v[-1] for k, v in self.counts.items()}, "iterations", seen["off"][2:4])
        self.compare(what, download_accel)
        return seen["off"]

    def state(self, k, download_accel=True):
        ctx = self.ctx[k]
        d = ctx.download()
        out = {f: bits(d[f]) for f in ("pos", "vel", "density")}
        out["ids"] = d["ids"]
        out["kappa"] = bits(ctx.download_solver_state()["kappa"])
        out["cell_first"], out["cell_idx"] = ctx.download_cells()
        if download_accel:
            out["accel"] = bits(ctx.download_accel())
        return out

    def compare(self, what="", download_accel=True):
        ref = self.state("off", download_accel)
        for k in self.ctx:
            if k == "off":
                continue
            got = self.state(k, download_accel)
            for f, a in ref.items():
                assert np.array_equal(got[f], a), f"{what}: {k} {f}"
        if self.o:
            d = self.ctx["off"].download()
            np.testing.assert_array_equal(d["ids"], self.o.ids(), what + " ids")
            assert_bits_equal(d["pos"], self.o.positions(), what + " positions")
            assert_bits_equal(d["vel"], self.o.velocities(), what + " velocities")
            assert_bits_equal(d["density"], self.o.densities(), what + " densities")
            assert_bits_equal(self.ctx["off"].download_solver_state()["kappa"], self.o.kappa(), what + " kappa")
        for k in ("off", "fill"):
            if k in self.ctx:
                assert self.ctx[k].rigid_predict_counts() == ZERO, f"{k}: the launches from before"

    def run(self, steps, what=""):
        return [self.step(f"{what} step {s}") for s in range(steps)]


@pytest.mark.parametrize("n", [N, 200, 257, 1024])
def test_block_in_free_fall_every_workgroup_exits(monkeypatch, n):
    """No boundary in reach: from the second step on every workgroup of the forced context's producer leaves through the exit, every
    workgroup of the accel context's walks with K.a; the hinted context follows once its hints stand (the rigid pass from the end of
    step 2, test_gpu_rigid_motion_skip).  n = 200: one ragged block; 257: a block of one particle; 1024: whole blocks only."""
    pos, vel = block(n, v=(0.25, 0.0))
    q = Quint(monkeypatch, pos, vel)
    nb = blocks_of(n)
    for s in range(6):
        st = q.step(f"n {n} step {s}")
        assert st[2:4] == (1, 1)
        acc = q.ctx["forced"].download_accel()
        assert uniform(acc) and acc[0, 0] == 0 and not np.signbit(acc[0, 0]) and abs(acc[0, 1] + 9.81) < 1e-5, acc[0]
    assert q.counts["forced"] == [ZERO] + [(1, nb, 0, 0)] * 5, q.counts
    assert q.counts["accel"] == [ZERO] + [(1, 0, nb, 0)] * 5, q.counts
    assert q.counts["on"][-2:] == [(1, nb, 0, 0)] * 2 and q.counts["on"][0] == ZERO, q.counts
    assert q.rigid["forced"] == [(1, 1, 0)] * 6 and q.rigid["fill"] == [(1, 1, 0)] * 6


def test_boundary_row_in_reach_then_the_quiet_end(monkeypatch):
    """The patch of tests/test_gpu_quiet_scene.py: a boundary row inside h of the lowest fluid rows.  While the scene is quiet the
    workgroups that walk (with K.a) are exactly the blocks that hold a particle with a static neighbour — from the oracle's neighbour
    counts of the lists the launch reads — and the others exit.  In step 2 the density loop has factors: the pass queued behind that
    step finds the marks and fills accel[], the new form queued in step 3 finds no verdict and reads the array, and the hinted context
    queues no rigid form afterwards."""
    pos, boundary = patch_scene(N)
    q = Quint(monkeypatch, pos, boundary=boundary)
    nb = blocks_of(N)
    marked_at = None
    for s in range(5):
        cnt, _, _ = q.o.neighbors()  # (the lists of the build behind the step before: what this step's first producer reads)
        walking = len(np.unique(np.nonzero(cnt[:, 0] != cnt[:, 1])[0] // 256)) if s else 0
        q.step(f"step {s}")
        if marked_at is None and np.any(q.o.kappa() != 0):
            marked_at = s
        if 1 <= s <= 2:
            assert 0 < walking < nb, walking
            assert q.counts["forced"][s] == (1, nb - walking, walking, 0), (s, q.counts, walking)
            assert q.counts["accel"][s] == (1, 0, nb, 0), (s, q.counts)
    assert marked_at == 2, marked_at
    assert q.rigid["forced"][2] == (1, 0, 1), q.rigid
    assert q.counts["forced"][3] == (1, 0, 0, 1) and q.counts["accel"][3] == (1, 0, 0, 1), q.counts
    # (the hinted context queues its one rigid pass behind step 2, marked: whichever form its producer has in step 3, nothing exits)
    assert all(c[1:3] == (0, 0) for c in q.counts["on"]) and q.counts["on"][:3] == [ZERO] * 3 and q.counts["on"][4] == ZERO, q.counts
    assert q.rigid["on"][2:] == [(1, 0, 1), (0, 0, 0), (0, 0, 0)], q.rigid


@pytest.mark.parametrize("gravity", [(0.0, -9.81), (-3e-43, -9.81)])
def test_one_particle_with_another_velocity_takes_the_slow_path(monkeypatch, gravity):
    """Every forced pass finds the gather's mark and fills accel[]; every launch of the new form finds no verdict.  The second case is
    the -0 against +0 scene of test_gpu_rigid_motion_skip: a denormal K.a.x whose a.x dt is -0, one particle with x velocity -0."""
    pos, vel = block()
    odd = int(sorted_ids(pos)[N // 2 + 7])
    vel[odd, 0] = np.float32(-0.0) if gravity[0] else np.float32(1e-3)
    q = Quint(monkeypatch, pos, vel, gravity=gravity)
    q.run(4)
    assert not uniform(q.o.velocities())
    assert q.rigid["forced"] == [(1, 0, 1)] * 4, q.rigid
    for k in ("forced", "accel"):
        assert q.counts[k] == [ZERO] + [(1, 0, 0, 1)] * 3, q.counts
    assert q.counts["on"] == [ZERO] * 4, q.counts


def test_wide_wavefronts_never_exit(monkeypatch):
    """list_span_limit = LISTS_32BIT: every wavefront keeps 32-bit global slots and gathers from global memory — with K.a from the
    arguments, in every workgroup."""
    pos, vel = block(v=(0.0, -0.125))
    q = Quint(monkeypatch, pos, vel, span=y.LISTS_32BIT)
    q.run(4)
    nb = blocks_of(N)
    assert q.counts["forced"] == [ZERO] + [(1, 0, nb, 0)] * 3, q.counts
    assert q.counts["accel"] == [ZERO] + [(1, 0, nb, 0)] * 3, q.counts


def test_physical_viscosity_model(monkeypatch):
    """k_nonpressure_rigid<PHYSICAL> in front of the new form; the device contexts against one another (the oracle has no such model)."""
    pos, vel = block(v=(0.0, -0.125))
    q = Quint(monkeypatch, pos, vel, viscosity="physical", oracle=False, names=("forced", "accel", "off"))
    q.run(4, "physical")
    nb = blocks_of(N)
    assert q.counts["forced"] == [ZERO] + [(1, nb, 0, 0)] * 3, q.counts
    assert q.counts["accel"] == [ZERO] + [(1, 0, nb, 0)] * 3, q.counts


def test_density_warm_start_reads_a_materialised_array(monkeypatch):
    """fixed_iterations = (2, 1): a warm start stands in front of the density loop, so the prediction is a k_predict of its own
    (launch_predict).  The rigid passes leave accel[] unwritten all the same; the fill goes in front of the prediction, the new form is
    never queued, and the bits are the off context's."""
    pos, vel = block(v=(0.1, 0.0))
    q = Quint(monkeypatch, pos, vel, fixed=(2, 1))
    # (no debug download here: the fill in front of k_predict is the only one)
    for s in range(4):
        st = q.step(f"step {s}", download_accel=False)
        assert st[2:4] == (2, 1)
    assert all(c == [ZERO] * 4 for c in q.counts.values()), q.counts
    assert sum(r[1] for r in q.rigid["forced"]) > 0, "rigid passes left the array to the fill"
    q.compare("end", download_accel=True)


@pytest.mark.parametrize("event", ["none", "download_accel", "upload", "append", "remove", "state"])
def test_events_between_the_run_ahead_pass_and_the_next_step(monkeypatch, event):
    """Three steps (the forced context's run-ahead pass is rigid and has left accel[] unwritten), the event in both contexts, three
    more: bit-equal to the off context all along.  none: no debug download at all in between — the exit's own course.  state: saved,
    and loaded into a fresh context that goes on in the old one's place."""
    pos, vel = block(v=(0.0, -0.5))
    q = Quint(monkeypatch, pos, vel, oracle=False, names=("forced", "off"))
    plain = event == "none"
    for s in range(3):
        q.step(f"before step {s}", download_accel=not plain)
    assert q.counts["forced"][-1] == (1, blocks_of(N), 0, 0), q.counts
    for k in list(q.ctx):
        ctx = q.ctx[k]
        if event == "download_accel":
            a = ctx.download_accel()
            assert uniform(a) and abs(a[0, 1] + 9.81) < 1e-5
        elif event == "upload":
            d = ctx.download()
            ctx.clear_cached()
            ctx.upload(d["pos"], d["vel"])
            q.timer[k] = y.TimeManager()
        elif event == "append":
            d = ctx.download()
            ctx.append(pos[:300] - np.float32([0.0, 0.3]), np.tile(d["vel"][:1], (300, 1)))
        elif event == "remove":
            assert ctx.remove((0.0, 0.0, 0.55, 10.0)) > 0
        elif event == "state":
            blob = ctx.save_state()
            fresh = make_ctx(monkeypatch, ENVS[k], pos[:10], None, None, (0, 0), (0.0, -9.81), "xsph", 0)
            fresh.load_state(blob)
            q.ctx[k] = fresh
    # (append reallocates the particle arrays and the state went into a fresh context: no pass has written that accel[] yet, with or
    # without the record, and there is nothing to compare before the next step's pass)
    q.compare("after " + event, download_accel=event not in ("none", "append", "state"))
    for s in range(3):
        q.step(f"after {event} step {s}", download_accel=not plain)
    assert q.counts["forced"][-1] == (1, blocks_of(len(q.ctx["off"].download()["pos"])), 0, 0), q.counts
