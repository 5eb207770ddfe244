"""The quiet take-over: under a loop's quiet hint the producer of the first iteration's factors finishes the
correction's per-particle work, and the first correction is queued in the thin form — one resident generation of workgroups that look
at the marks once and, in a quiet scene, touch no particle word.
  divergence loop: the neighbour build (or compute_density_change with SPHX_FUSE_DIV=0 or behind a warm start) stores stiffness = 0 + k;
  density loop:    compute_density_error stores kappa = 0 + k and makes the next build's cell count from p + v* dt, speculatively, its
                   flags waiting in a word of their own; the thin correction merges them (quiet) or drops them and recounts (marked).
With a mark set every thin workgroup runs the per-workgroup decision over its virtual blocks.

Every scene runs three ways in lock step — take-over on (the default wherever flags exist), SPHX_ZERO_SKIP=0 (no flags, so no
take-over) and the CPU oracle — with the bit-for-bit comparison of tests/test_gpu_zero_correction_skip.py (positions, velocities,
densities, kappa, stiffness, ids, both cell arrays, lists; dt in ns, iteration counts, warm-start decisions) and equal step flags.
The bookkeeping of tests/test_gpu_quiet_scene.py holds unchanged: a thin workgroup that leaves quietly counts as the blocks it
stands for.  sphx_debug_takeover_counts -> (thin launches, producers that took over, particles whose cell the recount moved): each
loop has one first iteration per step, so the first two read hint_d + hint_v of the step's start (hint_d only where the density
correction counts cells), and nothing moves in a step whose density loop stays quiet.

Fringe flag: the helpers here cannot bring a quiet patch to the fringe of the directory's cover within a few steps (a 64-cell block
is 1.28 m; free fall covers that in half a second of simulated time, thousands of steps), so DF_NEAR_EDGE through the speculative
word has no test of its own; the step flags are compared in every step of every scene instead.
"""
import numpy as np
import pytest
from test_gpu_quiet_scene import QuietTrio, blocks_of, host_step, patch_scene
from test_gpu_random_scenes import scene as random_scene
from test_gpu_zero_correction_skip import DIAM, Trio, make_ctx, remote_veto_scene
from util import assert_bits_equal, dam_break, lattice_scene

import yasph2d_amd as y

pytestmark = pytest.mark.gpu


def record_flags(ctx, log):
    """every step_finish of ctx appends its step flags to log"""
    inner = ctx.step_finish

    def step_finish(dt):
        st = inner(dt)
        log.append(st["flags"])
        return st

    ctx.step_finish = step_finish


class TakeTrio(QuietTrio):
    """QuietTrio + the take-over counters of the switch-on context per step, and the step flags of both contexts"""

    def __init__(self, monkeypatch, pos, vel=None, boundary=None, fixed=(0, 0), env=None):
        super().__init__(monkeypatch, pos, vel, boundary, fixed, env)
        env = env or {}
        # (the density loop's thin form needs the fused cell count; the second switch takes it out alone)
        self.density_thin = "SPHX_NO_FUSED_COUNT" not in env and env.get("SPHX_QUIET_TAKEOVER_DENSITY") != "0"
        self.take = []
        self.flags_on, self.flags_off = [], []
        record_flags(self.on, self.flags_on)
        record_flags(self.off, self.flags_off)

    def expect_take(self, t0, what):
        D, hint_d, hint_v = self.log[-1][0], self.log[-1][6], self.log[-1][7]  # (the hints the step started with)
        self.take.append(tuple(b - a for a, b in zip(t0, self.on.takeover_counts())))
        print(what, "take-over (thin, producers, moved)", self.take[-1])
        want = int(hint_v) + int(hint_d and self.density_thin)
        assert self.take[-1][:2] == (want, want), (what, self.take, self.log[-1])
        assert self.take[-1][2] == 0 or D, (what, "a quiet density loop moves nothing", self.take)
        assert self.flags_on[-1] == self.flags_off[-1], (what, self.flags_on, self.flags_off)
        assert self.off.takeover_counts() == (0, 0, 0), "no flags, no take-over"

    def step(self, what=""):
        t0 = self.on.takeover_counts()
        st = super().step(what)
        self.expect_take(t0, what)
        return st


def zero_bits(t):
    ss = t.on.download_solver_state()
    return not ss["kappa"].view(np.uint32).any() and not ss["stiffness"].view(np.uint32).any()


def test_lattice_runs_the_thin_form_from_the_second_step(monkeypatch):
    """~20 k particles of reset_fluid: step 0 has no hint and queues nothing new; from step 1 on the build stores the stiffness and the
    divergence correction is thin.  The quiet-scene counters read what they read before: a thin workgroup stands for its blocks."""
    pos, boundary = dam_break(float(np.sqrt(20000 / 4050)))
    t = TakeTrio(monkeypatch, pos, boundary=boundary)
    t.run(6)
    blocks = blocks_of(len(pos))
    assert t.take == [(0, 0, 0)] + [(2, 2, 0)] * 5, t.take
    assert [e[4:6] for e in t.log] == [(0, 0)] + [(2 * blocks, 2)] * 5, t.log
    assert t.on.correction_counts() == (6 * 2 * blocks, 0, 0)
    assert t.on.takeover_counts() == (10, 10, 0)
    assert zero_bits(t), "+0, not -0"


@pytest.mark.parametrize("grid", [None, 1, 3])
@pytest.mark.parametrize("n", [1, 63, 64, 255, 256, 257, 1000])
def test_sizes_at_the_edges(monkeypatch, n, grid):
    """One workgroup and a few, ragged last wavefronts and workgroups, and the grid of 256-particle blocks rounded up to a multiple of
    eight: with SPHX_THIN_GRID=1 one workgroup stands for all of them, the empty ones included, with 3 (n = 1000: eight blocks) they
    split 3, 3 and 2.  In step 2 the density loop is marked while its hint is set: the speculative count is followed by the marked thin
    path and its recount, while the divergence loop stays quiet and thin in the same step."""
    pos, boundary = patch_scene(n)
    t = TakeTrio(monkeypatch, pos, boundary=boundary, env={"SPHX_THIN_GRID": str(grid)} if grid else None)
    t.run(4, f"n={n} grid={grid}")
    b = blocks_of(n)
    assert [e[4:6] for e in t.log[:2]] == [(0, 0), (2 * b, 2)], t.log
    assert t.take[:2] == [(0, 0, 0), (2, 2, 0)] and t.take[2][:2] == (2, 2), t.take
    if n > 1:
        assert t.log[2][:2] == (True, False) and t.log[2][4:] == (b, 2, True, True), t.log


def forced_trio(monkeypatch, pos, vel=None, boundary=None, fixed=(0, 0), grid="2"):
    monkeypatch.setenv("SPHX_QUIET_TAKEOVER", "force")
    monkeypatch.setenv("SPHX_THIN_GRID", grid)
    t = Trio(monkeypatch, pos, vel, boundary, fixed)
    monkeypatch.delenv("SPHX_QUIET_TAKEOVER")
    monkeypatch.delenv("SPHX_THIN_GRID")
    t.flags_on, t.flags_off = [], []
    record_flags(t.on, t.flags_on)
    record_flags(t.off, t.flags_off)
    return t


@pytest.mark.parametrize("grid", ["2", "3"])
def test_forced_on_the_disturbed_patch(monkeypatch, grid):
    """remote_veto_scene under SPHX_QUIET_TAKEOVER=force with two or three thin workgroups (32 blocks: 16 and 16, or the ragged 11, 11
    and 10): every first iteration of both loops is a thin launch that finds the mark, and each workgroup runs the decision — skip,
    window flag, remote entry — over its share of the blocks, the density loop's ending in the recount."""
    pos, _ = remote_veto_scene()
    t = forced_trio(monkeypatch, pos, grid=grid)
    corrects = False
    for s in range(3):
        t.step(f"step {s}")
        t.compare(f"step {s}")
        assert t.flags_on[-1] == t.flags_off[-1]
        corrects |= bool(np.any(t.o.stiffness() != 0))
    assert corrects, "the divergence loop really corrects"
    print("take-over", t.on.takeover_counts())
    assert t.on.takeover_counts()[:2] == (6, 6)
    assert t.on.takeover_counts()[2] > 0, "the recount moved a particle"
    skipped, window, remote = t.on.correction_counts()
    print("skipped, window, remote", skipped, window, remote)
    assert skipped > 0 and window > 0, (skipped, window, remote)
    assert t.on.quiet_counts()[0] == 0, "nobody leaves a marked scene quietly"


def test_forced_on_a_random_cloud(monkeypatch):
    """Seed 15 of tests/test_gpu_random_scenes.py (blobs with random velocities over floor pieces, fixed iterations (2, 2), a fixed
    50 us step; chosen by running the build: its recount moves a particle in step 0 already, seeds 6 and 8 move none at this step).
    Step 0's divergence producer is the neighbour build, from step 1 on the loop starts with a warm start and compute_density_change
    is the producer; the second iterations run the form without take-over behind a thin first one and wipe the speculative count."""
    pos, vel, boundary = random_scene(15)
    t = forced_trio(monkeypatch, pos, vel, boundary, fixed=(2, 2))
    t.t_on, t.t_off = y.TimeManager(fixed_ns=50_000), y.TimeManager(fixed_ns=50_000)
    t.o.timer_fixed(50_000)
    corrects = 0
    for s in range(4):
        st = t.step(f"step {s}")
        t.compare(f"step {s}")
        assert t.flags_on[-1] == t.flags_off[-1]
        assert st["divergence_iterations"] == 2 and st["warmstart_divergence"] == (1 if s else 0)
        corrects += int(np.count_nonzero(t.o.stiffness()))
    assert corrects > 0, "the divergence loop really corrects"
    assert np.any(t.o.kappa() != 0), "and so does the density loop"
    print("take-over", t.on.takeover_counts())
    assert t.on.takeover_counts()[:2] == (8, 8)
    assert t.on.takeover_counts()[2] > 0, "the recount moved a particle: the atomicSub / atomicAdd pair ran"


def test_fixed_iterations_run_the_old_form_behind_a_thin_first_one(monkeypatch):
    """fixed_iterations = (2, 2) on the lattice: the loop starts with a warm start, so compute_density_change is the producer that
    takes the store over; the second iteration reads the sum the producer stored and adds its own k.  All of it +0."""
    pos, boundary = dam_break(float(np.sqrt(20000 / 4050)))
    t = TakeTrio(monkeypatch, pos, boundary=boundary, fixed=(2, 2))
    t.run(4)
    assert t.take == [(0, 0, 0)] + [(2, 2, 0)] * 3, t.take
    assert [e[4] for e in t.log] == [0] + [4 * blocks_of(len(pos))] * 3, t.log
    assert zero_bits(t), "+0, not -0"


@pytest.mark.parametrize("env", [{"SPHX_FUSE_DIV": "0"}, {"SPHX_NO_FUSED_COUNT": "1"}, {"SPHX_HOST_LOOP": "1"}, {"SPHX_QUIET_TAKEOVER_DENSITY": "0"}],
                         ids=lambda e: "-".join(e))
def test_other_producers_and_drivers(monkeypatch, env):
    """SPHX_FUSE_DIV=0: compute_density_change is the divergence loop's producer in every step; SPHX_NO_FUSED_COUNT=1: no speculative
    count, so the density correction is not thin; SPHX_HOST_LOOP=1: every first iteration drops the count of the step before, which
    must happen in front of the compute_density_error that makes the new one; SPHX_QUIET_TAKEOVER_DENSITY=0: the divergence part alone."""
    pos, boundary = patch_scene(1000)
    t = TakeTrio(monkeypatch, pos, boundary=boundary, env=env)
    t.run(4, "-".join(env))
    k = 2 if t.density_thin else 1
    assert t.take[:2] == [(0, 0, 0), (k, k, 0)] and t.take[2][:2] == (k, k), t.take


def test_step_begin_without_a_timer_law(monkeypatch):
    pos, boundary = patch_scene(1000)
    t = TakeTrio(monkeypatch, pos, boundary=boundary)
    for s in range(4):
        q0, t0 = t.on.quiet_counts(), t.on.takeover_counts()
        st = host_step(t, False, f"step {s}")
        t.expect(st, q0, t.on.quiet_counts(), f"step {s}")
        t.expect_take(t0, f"step {s}")
        t.compare(f"step {s}")
    assert t.take[:2] == [(0, 0, 0), (2, 2, 0)] and t.take[2][:2] == (2, 2), t.take


def test_switch_off_queues_the_parents_launches(monkeypatch):
    """SPHX_QUIET_TAKEOVER=0: the decide-first forms run as before, nothing is thin, nobody takes a store over."""
    pos, boundary = dam_break(float(np.sqrt(20000 / 4050)))
    t = QuietTrio(monkeypatch, pos, boundary=boundary, env={"SPHX_QUIET_TAKEOVER": "0"})
    t.run(3)
    assert t.on.takeover_counts() == (0, 0, 0)
    assert t.on.quiet_counts() == (2 * 2 * blocks_of(len(pos)), 4)


def test_upload_between_quiet_steps(monkeypatch):
    """quiet lattice -> the disturbed scene -> the lattice again on the same contexts: the first step behind an upload has no hint, so
    nothing is thin in it; TakeTrio.step asserts that in every step."""
    quiet, _ = lattice_scene(5000, 0)
    disturbed, _ = remote_veto_scene()
    t = TakeTrio(monkeypatch, quiet)
    t.run(3, "quiet")
    t.upload(disturbed)
    t.run(2, "disturbed")
    t.upload(quiet)
    t.run(3, "quiet again")
    assert t.take == [(0, 0, 0), (2, 2, 0), (2, 2, 0)] + [(0, 0, 0)] * 2 + [(0, 0, 0), (2, 2, 0), (2, 2, 0)], t.take


def steps(ctx, timer, k):
    for _ in range(k):
        vmax = ctx.step_begin(timer.simulation_step(), timer.law(DIAM))
        ctx.step_finish(y.duration_as_secs_f32(timer.update_simulation_step(DIAM, vmax)))


def make_pair(monkeypatch, pos, boundary):
    """the same scene with take-over on and with SPHX_QUIET_TAKEOVER=0, flags on in both"""
    a = make_ctx(monkeypatch, True, pos, None, boundary)
    monkeypatch.setenv("SPHX_QUIET_TAKEOVER", "0")
    b = make_ctx(monkeypatch, True, pos, None, boundary)
    monkeypatch.delenv("SPHX_QUIET_TAKEOVER")
    return a, b


def test_append_between_quiet_steps(monkeypatch):
    """sphx_append drops the hints: the step behind it queues nothing thin, and the run ends with the digest of the run without take-over."""
    pos, boundary = dam_break(float(np.sqrt(20000 / 4050)))
    extra, _ = lattice_scene(300, 0, origin=(pos[:, 0].min(), pos[:, 1].max() + 0.2))
    a, b = make_pair(monkeypatch, pos, boundary)
    ta, tb = y.TimeManager(), y.TimeManager()
    steps(a, ta, 3)
    steps(b, tb, 3)
    assert a.takeover_counts() == (4, 4, 0) and b.takeover_counts() == (0, 0, 0)
    assert a.append(extra) == b.append(extra)
    steps(a, ta, 1)
    steps(b, tb, 1)
    assert a.takeover_counts() == (4, 4, 0), "no hint behind an edit"
    steps(a, ta, 2)
    steps(b, tb, 2)
    assert a.takeover_counts() == (8, 8, 0) and b.takeover_counts() == (0, 0, 0)
    assert a.state_digest() == b.state_digest()
    sa, sb = a.download_solver_state(), b.download_solver_state()
    for k in ("kappa", "stiffness"):
        assert np.array_equal(sa[k].view(np.uint32), sb[k].view(np.uint32)), k


def test_save_load_and_step_on(monkeypatch):
    """No part of the take-over is state: a run that saves, loads and steps on ends with the digest of an uninterrupted run and of a
    run without take-over, and its first step behind the load queues nothing thin."""
    pos, boundary = dam_break(float(np.sqrt(20000 / 4050)))
    a, off = make_pair(monkeypatch, pos, boundary)
    b = make_ctx(monkeypatch, True, pos, None, boundary)
    ta, tb, toff = y.TimeManager(), y.TimeManager(), y.TimeManager()
    steps(a, ta, 5)
    steps(off, toff, 5)
    steps(b, tb, 3)
    assert b.takeover_counts() == (4, 4, 0)
    b.load_state(b.save_state())
    steps(b, tb, 1)
    assert b.takeover_counts() == (4, 4, 0), "no hint behind a load"
    steps(b, tb, 1)
    assert b.takeover_counts() == (6, 6, 0)
    assert a.takeover_counts() == (8, 8, 0) and off.takeover_counts() == (0, 0, 0)
    assert a.state_digest() == b.state_digest() == off.state_digest()
    da, db = a.download(), b.download()
    for k in ("pos", "vel", "density"):
        assert_bits_equal(da[k], db[k], k)


def test_nan_velocity_after_quiet_steps(monkeypatch):
    """Two quiet steps, then the lattice comes back with one NaN velocity: the upload drops the hints, the failing step queues nothing
    thin and leaves the bits of a context without flags; the context recovers with a fresh upload and starts without a hint."""
    pos, boundary = dam_break(float(np.sqrt(20000 / 4050)))
    vel = np.zeros_like(pos)
    vel[len(pos) // 2, 0] = np.float32("nan")
    out = []
    for skip in (True, False):
        ctx = make_ctx(monkeypatch, skip, pos, None, boundary)
        timer = y.TimeManager()
        steps(ctx, timer, 2)
        k = ctx.takeover_counts()
        assert k == ((2, 2, 0) if skip else (0, 0, 0))
        ctx.clear_cached()
        ctx.upload(pos, vel)
        timer = y.TimeManager()
        with pytest.raises(y.SphxError) as e:
            ctx.step_begin(timer.simulation_step(), timer.law(DIAM))
        assert e.value.code == y._lib.ERR_NONFINITE
        assert ctx.takeover_counts() == k
        d, ss = ctx.download(), ctx.download_solver_state()
        out.append((d["pos"], d["vel"], d["density"], ss["kappa"], ss["stiffness"]))
        if skip:
            ctx.clear_cached()
            ctx.upload(pos)
            timer = y.TimeManager()
            steps(ctx, timer, 1)
            assert ctx.takeover_counts() == k
            steps(ctx, timer, 1)
            assert ctx.takeover_counts() == (4, 4, 0)
    for a, b in zip(*out):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_two_tiles_never_see_it(monkeypatch):
    """The lattice on two tiles, contexts created with the switches on (forced, even): a tile's corrections get no flags, so all three
    counters stay 0 and the run equals the oracle-backed tile run."""
    from test_gpu_multi import oracle_tiles
    from test_tiles_cpu import run_tiles_threaded
    from tiles_reference import GpuTileBackend, cell_coord, quantile_cuts

    pos, boundary = dam_break(1.0)
    n_steps = 4
    cuts = quantile_cuts(cell_coord(pos, 1), 2)
    kw = dict(halo=16, cuts=cuts, adaptive_halo=True, rebalance_every=8)
    o, _ = oracle_tiles(pos, boundary, 2, 1, n_steps, **kw)
    for k, v in (("SPHX_ZERO_SKIP", "1"), ("SPHX_ZERO_SKIP_COUNT", "1"), ("SPHX_QUIET_TAKEOVER", "force"), ("SPHX_THIN_GRID", "2")):
        monkeypatch.setenv(k, v)
    ctxs = [y.SphxContext(), y.SphxContext()]
    for k in ("SPHX_ZERO_SKIP", "SPHX_ZERO_SKIP_COUNT", "SPHX_QUIET_TAKEOVER", "SPHX_THIN_GRID"):
        monkeypatch.delenv(k)
    g, _ = run_tiles_threaded(lambda r: GpuTileBackend(ctxs[r]), pos, boundary, 2, 1, n_steps, **kw)
    for r in range(2):
        np.testing.assert_array_equal(g[r][0]["ids"], o[r][0]["ids"])
        for k in ("pos", "vel", "density", "kappa"):
            assert_bits_equal(g[r][0][k], o[r][0][k], f"rank {r} {k}")
        assert ctxs[r].takeover_counts() == (0, 0, 0) and ctxs[r].quiet_counts() == (0, 0)
