"""The quiet-scene exit of k_correct: when no particle of the scene has a correction factor other than +-0, a
correction launched in the decide-first form reads one mark per stripe and leaves before it has requested a list word.

Every scene runs three ways in lock step — switch on (SPHX_ZERO_SKIP=1, counters collected), SPHX_ZERO_SKIP=0 and the CPU oracle —
with the bit-for-bit comparison of tests/test_gpu_zero_correction_skip.py (positions, velocities, densities, kappa, stiffness, ids,
both cell arrays, neighbour lists; dt in ns, iteration counts, warm-start decisions).  The counters show which path ran:
sphx_debug_quiet_counts -> (workgroups that left through the quiet exit, corrections the host queued in the decide-first form).

What the counters must read follows from the oracle.  Every k is err * alpha with err >= 0 and alpha > 0, so a loop's warm-start sum
(kappa / stiffness, started from zero in each step) has a non-zero entry exactly when some iteration of the loop produced a k != 0:
that is "the loop's mark was set" (D for the density loop, V for the divergence loop).  The host's hint for a loop is what its
terminating correction of the step before saw, and it is dropped by an upload, a load or a failed step:

    decide-first launches of a step  = Id * hint_d + Iv * hint_v      (Id, Iv: the step's iteration counts)
    quiet exits of a step            = blocks * (Id * (hint_d and not D) + Iv * (hint_v and not V))
    hints after the step             = (not D, not V)

(The launch count is exact when the step needs as many iterations as the step before, which the device-run loop queues up front; a
loop that needs more queues one iteration past the last, which returns at once but was launched.)
"""
import numpy as np
import pytest
from test_gpu_zero_correction_skip import DIAM, Trio, make_ctx, remote_veto_scene
from util import assert_bits_equal, dam_break, lattice_scene

import yasph2d_amd as y

pytestmark = pytest.mark.gpu


def blocks_of(n):
    return (n + 255) // 256


class QuietTrio(Trio):
    """Trio + the bookkeeping of the module docstring for the switch-on context"""

    def __init__(self, monkeypatch, pos, vel=None, boundary=None, fixed=(0, 0), env=None):
        for k, v in (env or {}).items():
            monkeypatch.setenv(k, v)
        super().__init__(monkeypatch, pos, vel, boundary, fixed)
        for k in env or {}:
            monkeypatch.delenv(k)
        self.mp, self.fixed, self.boundary = monkeypatch, fixed, boundary
        self.n = len(pos)
        self.hint = [False, False]
        self.prev_iters = None
        self.log = []  # per step: (D, V, Id, Iv, quiet exits, decide-first launches, hint_d, hint_v before the step)

    def upload(self, pos, vel=None):
        """another scene on the same contexts: fresh oracle, fresh timers, hints gone"""
        from test_gpu_zero_correction_skip import make_oracle

        for c in (self.on, self.off):
            c.clear_cached()
            c.upload(pos, vel)
        self.o = make_oracle(pos, vel, self.boundary, self.fixed)
        self.t_on, self.t_off = y.TimeManager(), y.TimeManager()
        self.n = len(pos)
        self.hint = [False, False]
        self.prev_iters = None

    def expect(self, st, q0, q1, what):
        D, V = bool(np.any(self.o.kappa() != 0)), bool(np.any(self.o.stiffness() != 0))
        Id, Iv = st["density_iterations"], st["divergence_iterations"]
        quiet, launches = q1[0] - q0[0], q1[1] - q0[1]
        self.log.append((D, V, Id, Iv, quiet, launches, self.hint[0], self.hint[1]))
        print(what, "D V Id Iv", D, V, Id, Iv, "hints", self.hint, "quiet exits", quiet, "decide-first launches", launches)
        hd, hv = self.hint
        assert quiet == blocks_of(self.n) * (Id * (hd and not D) + Iv * (hv and not V)), (what, self.log[-1], self.hint)
        want = Id * hd + Iv * hv
        if want == 0 or self.prev_iters == (Id, Iv):
            assert launches == want, (what, self.log[-1], self.hint)
        else:
            assert want <= launches <= want + 2, (what, self.log[-1], self.hint)
        self.hint = [not D, not V]
        self.prev_iters = (Id, Iv)

    def step(self, what=""):
        q0 = self.on.quiet_counts()
        st = super().step(what)
        self.expect(st, q0, self.on.quiet_counts(), what)
        assert self.off.quiet_counts() == (0, 0), "SPHX_ZERO_SKIP=0 hands no flags to any correction"
        return st

    def run(self, steps, what=""):
        for s in range(steps):
            self.step(f"{what} step {s}")
            self.compare(f"{what} step {s}")


def host_step(t, law, what):
    """One step of all three with step_begin's plain form (law = False: the host derives dt and starts phase B) or the law form."""
    so = t.o.dfsph_step()
    out = None
    for ctx, timer in ((t.on, t.t_on), (t.off, t.t_off)):
        vmax = ctx.step_begin(timer.simulation_step(), timer.law(DIAM) if law else None)
        dt_ns = timer.update_simulation_step(DIAM, vmax)
        st = ctx.step_finish(y.duration_as_secs_f32(dt_ns))
        assert dt_ns == t.o.timer_step_ns(), what
        for k in ("density_iterations", "divergence_iterations", "warmstart_density", "warmstart_divergence", "neighbor_entries"):
            assert st[k] == so[k], (what, k, st[k], so[k])
        out = out or st
    return out


def patch_scene(n):
    """n lattice particles (8 neighbours inside h = 0.02: densities below rho0, every factor zero) and a boundary row 0.019 below the
    lowest fluid row: in reach of it, too far to lift a density over rho0 — until the patch has fallen towards it for two steps."""
    pos, b = lattice_scene(n, 64)
    b = b.copy()
    b[:, 1] = np.float32(0.5) - np.float32(0.019)
    return pos, b


def test_lattice_leaves_through_the_quiet_exit_from_the_second_step(monkeypatch):
    """~20 k particles of reset_fluid: the first step has no hint and skips workgroup by workgroup; from the second step on every
    workgroup of both corrections leaves through the quiet exit.  A quiet exit is a skip: the old counter still reads 6 * 2 * blocks."""
    pos, boundary = dam_break(float(np.sqrt(20000 / 4050)))
    t = QuietTrio(monkeypatch, pos, boundary=boundary)
    t.run(6)
    blocks = blocks_of(len(pos))
    assert all(e[:4] == (False, False, 1, 1) for e in t.log), t.log
    assert [e[4:6] for e in t.log] == [(0, 0)] + [(2 * blocks, 2)] * 5, t.log
    assert t.on.correction_counts() == (6 * 2 * blocks, 0, 0)
    assert t.on.quiet_counts() == (5 * 2 * blocks, 10)


def test_second_iteration_adds_the_factor_to_the_warm_start_sum(monkeypatch):
    """fixed_iterations = (2, 2): the second iteration of each loop is quiet with first = 0 — the warm-start word is read, k is added
    and the sum stored (all zeros: kappa and stiffness must stay +0 as the oracle's do)."""
    pos, boundary = dam_break(float(np.sqrt(20000 / 4050)))
    t = QuietTrio(monkeypatch, pos, boundary=boundary, fixed=(2, 2))
    t.run(4)
    blocks = blocks_of(len(pos))
    assert all(e[:4] == (False, False, 2, 2) for e in t.log), t.log
    assert [e[4] for e in t.log] == [0] + [4 * blocks] * 3, t.log
    assert [e[5] for e in t.log[2:]] == [4, 4], t.log
    assert t.on.correction_counts() == (4 * 4 * blocks, 0, 0)
    ss = t.on.download_solver_state()
    assert not ss["kappa"].view(np.uint32).any() and not ss["stiffness"].view(np.uint32).any(), "+0, not -0"


@pytest.mark.parametrize("n", [1, 63, 64, 255, 256, 257, 1000])
def test_sizes_at_the_edges(monkeypatch, n):
    """One workgroup and a few, full and ragged last wavefronts and workgroups.  Steps 0 and 1 are quiet; in step 2 the lowest row has
    come close enough to the boundary for a density factor: the density correction, queued in the decide-first form on step 1's
    hint, finds the mark and goes on into the per-workgroup decision, while the divergence loop (nothing moves relative to anything)
    stays quiet — one loop quiet, the other not, in one step.  Step 3 runs the density correction in the plain form again; what it
    must count follows from the oracle (module docstring)."""
    pos, boundary = patch_scene(n)
    t = QuietTrio(monkeypatch, pos, boundary=boundary)
    t.run(4, f"n={n}")
    b = blocks_of(n)
    assert [e[:2] for e in t.log[:2]] == [(False, False), (False, False)], t.log
    assert [e[4:6] for e in t.log[:2]] == [(0, 0), (2 * b, 2)], t.log
    if n > 1:  # (a single particle has no lowest row to feel the boundary first: it stays quiet)
        assert t.log[2][:2] == (True, False) and t.log[2][4:] == (b, 2, True, True), t.log


def test_disturbed_patch_takes_no_quiet_exit(monkeypatch):
    """The lattice with a compressed 5 x 5 patch (remote_veto_scene): both loops iterate on real factors in every step.  No hint is
    ever raised, no correction is queued in the decide-first form, and the per-workgroup skip still fires away from the patch."""
    pos, _ = remote_veto_scene()
    t = QuietTrio(monkeypatch, pos)
    t.run(3)
    assert all(e[0] and e[1] for e in t.log), t.log
    assert any(e[3] > 1 for e in t.log), ("the divergence loop iterates", t.log)
    assert t.on.quiet_counts() == (0, 0)
    skipped, window, remote = t.on.correction_counts()
    assert skipped > 0 and window > 0, (skipped, window, remote)


def test_transitions_on_one_context(monkeypatch):
    """quiet lattice -> upload of the disturbed scene -> the lattice again, on the same contexts: a mark or a hint left by the scene
    before must not reach the scene behind the upload.  The first step behind each upload queues no decide-first form."""
    quiet, _ = lattice_scene(5000, 0)
    disturbed, _ = remote_veto_scene()
    t = QuietTrio(monkeypatch, quiet)
    t.run(3, "quiet")
    assert t.log[-1][4:6] == (2 * blocks_of(len(quiet)), 2)
    k = len(t.log)
    t.upload(disturbed)
    t.run(3, "disturbed")
    assert all(e[4:6] == (0, 0) for e in t.log[k:]), t.log[k:]
    k = len(t.log)
    t.upload(quiet)
    t.run(3, "quiet again")
    assert [e[4:6] for e in t.log[k:]] == [(0, 0)] + [(2 * blocks_of(len(quiet)), 2)] * 2, t.log[k:]


def test_nan_velocity_after_quiet_steps(monkeypatch):
    """Two quiet steps raise both hints; then the lattice comes back with one NaN velocity.  The upload drops the hints, so the one
    density correction that runs before the step fails (tests/test_gpu_zero_correction_skip.py has the course of that step: every k
    is fmax(rho0, NaN) - rho0 = 0, a NaN k cannot be made through the interface) is the plain form, nobody takes the quiet exit, and
    what it leaves equals the switch-off context's bits.  The failed step leaves no hint either."""
    pos, boundary = dam_break(float(np.sqrt(20000 / 4050)))
    vel = np.zeros_like(pos)
    vel[len(pos) // 2, 0] = np.float32("nan")
    out = []
    for skip in (True, False):
        ctx = make_ctx(monkeypatch, skip, pos, None, boundary)
        timer = y.TimeManager()
        for _ in range(2):
            vmax = ctx.step_begin(timer.simulation_step(), timer.law(DIAM))
            ctx.step_finish(y.duration_as_secs_f32(timer.update_simulation_step(DIAM, vmax)))
        q = ctx.quiet_counts()
        assert q == ((2 * blocks_of(len(pos)), 2) if skip else (0, 0))
        ctx.clear_cached()
        ctx.upload(pos, vel)
        timer = y.TimeManager()
        with pytest.raises(y.SphxError) as e:
            ctx.step_begin(timer.simulation_step(), timer.law(DIAM))
        assert e.value.code == y._lib.ERR_NONFINITE
        assert ctx.quiet_counts() == q
        d, ss = ctx.download(), ctx.download_solver_state()
        out.append((d["pos"], d["vel"], d["density"], d["ids"], ss["kappa"], ss["stiffness"], ss["alpha"]))
        if skip:  # the context recovers with a fresh upload, and starts without a hint
            ctx.clear_cached()
            ctx.upload(pos)
            timer = y.TimeManager()
            vmax = ctx.step_begin(timer.simulation_step(), timer.law(DIAM))
            ctx.step_finish(y.duration_as_secs_f32(timer.update_simulation_step(DIAM, vmax)))
            assert ctx.quiet_counts() == q
    for a, b in zip(*out):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert np.isnan(out[0][1]).any()


@pytest.mark.parametrize("env", [{"SPHX_FUSE_DIV": "0"}, {"SPHX_NO_FUSED_COUNT": "1"}, {"SPHX_HOST_LOOP": "1"}], ids=lambda e: "-".join(e))
def test_other_producers_and_drivers(monkeypatch, env):
    """SPHX_FUSE_DIV=0: k_compute_error<true> produces the first divergence iteration's factors and mark, not the neighbour build;
    SPHX_NO_FUSED_COUNT=1: the density correction does not count cells; SPHX_HOST_LOOP=1: the host judges every residual."""
    pos, boundary = patch_scene(1000)
    t = QuietTrio(monkeypatch, pos, boundary=boundary, env=env)
    t.run(4, "-".join(env))
    assert [e[4:6] for e in t.log[:3]] == [(0, 0), (8, 2), (4, 2)] and t.log[2][:2] == (True, False), t.log


def test_step_begin_without_a_timer_law(monkeypatch):
    """phase B started by the host: no iteration is queued ahead, the density loop's first correction takes dt as an argument"""
    pos, boundary = patch_scene(1000)
    t = QuietTrio(monkeypatch, pos, boundary=boundary)
    for s in range(4):
        q0 = t.on.quiet_counts()
        st = host_step(t, False, f"step {s}")
        t.expect(st, q0, t.on.quiet_counts(), f"step {s}")
        t.compare(f"step {s}")
    assert [e[4:6] for e in t.log[:3]] == [(0, 0), (8, 2), (4, 2)] and t.log[2][:2] == (True, False), t.log


def test_save_load_and_step_on(monkeypatch):
    """The hint is no part of a state blob: a run that saves, loads and steps on ends with the digest of an uninterrupted run, and its
    first step behind the load queues no decide-first form."""
    pos, boundary = dam_break(float(np.sqrt(20000 / 4050)))
    blocks = blocks_of(len(pos))

    def steps(ctx, timer, k):
        for _ in range(k):
            vmax = ctx.step_begin(timer.simulation_step(), timer.law(DIAM))
            ctx.step_finish(y.duration_as_secs_f32(timer.update_simulation_step(DIAM, vmax)))

    a, b = make_ctx(monkeypatch, True, pos, None, boundary), make_ctx(monkeypatch, True, pos, None, boundary)
    ta, tb = y.TimeManager(), y.TimeManager()
    steps(a, ta, 5)
    steps(b, tb, 3)
    assert b.quiet_counts() == (2 * 2 * blocks, 4)
    dig = b.state_digest()
    b.load_state(b.save_state())
    assert b.state_digest() == dig
    steps(b, tb, 1)
    assert b.quiet_counts() == (2 * 2 * blocks, 4), "no hint behind a load"
    steps(b, tb, 1)
    assert b.quiet_counts() == (3 * 2 * blocks, 6)
    assert a.quiet_counts() == (4 * 2 * blocks, 8)
    assert a.state_digest() == b.state_digest()
    da, db = a.download(), b.download()
    for k in ("pos", "vel", "density"):
        assert_bits_equal(da[k], db[k], k)


def test_two_tiles_never_see_it(monkeypatch):
    """The lattice on two tiles, contexts created with the switch on: a tile's corrections get no flags, so both counters stay 0 and
    the run equals the oracle-backed tile run; sphx_multi, created under the same environment, equals it too."""
    from test_gpu_multi import compare, oracle_tiles
    from test_tiles_cpu import run_tiles_threaded
    from tiles_reference import GpuTileBackend, cell_coord, quantile_cuts
    from yasph2d_amd.multi import MultiSolver

    pos, boundary = dam_break(1.0)
    steps = 6
    cuts = quantile_cuts(cell_coord(pos, 1), 2)
    kw = dict(halo=16, cuts=cuts, adaptive_halo=True, rebalance_every=8)
    o, _ = oracle_tiles(pos, boundary, 2, 1, steps, **kw)
    monkeypatch.setenv("SPHX_ZERO_SKIP", "1")
    monkeypatch.setenv("SPHX_ZERO_SKIP_COUNT", "1")
    ctxs = [y.SphxContext(), y.SphxContext()]
    m = MultiSolver(y.default_params(), devices=[0, 0], halo=16, rebalance_every=8)
    monkeypatch.delenv("SPHX_ZERO_SKIP")
    monkeypatch.delenv("SPHX_ZERO_SKIP_COUNT")
    g, _ = run_tiles_threaded(lambda r: GpuTileBackend(ctxs[r]), pos, boundary, 2, 1, steps, **kw)
    for r in range(2):
        np.testing.assert_array_equal(g[r][0]["ids"], o[r][0]["ids"])
        for k in ("pos", "vel", "density", "kappa"):
            assert_bits_equal(g[r][0][k], o[r][0][k], f"rank {r} {k}")
        assert ctxs[r].quiet_counts() == (0, 0) and ctxs[r].correction_counts() == (0, 0, 0)
    m.set_strips(1, cuts)
    m.set_boundary(boundary)
    m.upload(pos)
    timer = y.TimeManager()
    stats = [m.step(timer) for _ in range(steps)]
    compare(m.download(), o, stats, o[0][1])
