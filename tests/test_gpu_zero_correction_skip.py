"""The zero-correction skip of k_correct: a correction workgroup whose whole reach has k = +-0 skips its walk.

Every scene runs three ways — a context with the switch on (the default, counters collected: SPHX_ZERO_SKIP_COUNT=1), a context with
SPHX_ZERO_SKIP=0 and the CPU oracle — and velocities, positions, kappa, stiffness, densities, ids, cell arrays and the step statistics
must agree bit for bit (the comparison of tests/test_gpu_parity.py).  The counters (sphx_debug_correction_counts: workgroups that
skipped / that a flag of their window stopped / that a flag behind an out-of-window table line or a wavefront in the wide list
format stopped) show that the path a test is about was really taken.
"""
import numpy as np
import pytest
from util import assert_bits_equal, assert_same_neighbors, dam_break

import yasph2d_amd as y
from oracle.oracle import Oracle

pytestmark = pytest.mark.gpu

DIAM = np.float32(0.01)
SPACING = np.float32(1.0 / 90.0)  # the reference's fluid lattice: 8 neighbours inside h = 0.02, density below rho0
STAT_KEYS = ("density_iterations", "divergence_iterations", "warmstart_density", "warmstart_divergence", "neighbor_entries")


def make_ctx(monkeypatch, skip, pos, vel=None, boundary=None, fixed=(0, 0)):
    """The switches are read once, in sphx_create."""
    monkeypatch.setenv("SPHX_ZERO_SKIP", "1" if skip else "0")
    monkeypatch.setenv("SPHX_ZERO_SKIP_COUNT", "1")
    ctx = y.SphxContext(y.default_params(fixed_iterations=fixed))
    monkeypatch.delenv("SPHX_ZERO_SKIP")
    monkeypatch.delenv("SPHX_ZERO_SKIP_COUNT")
    if boundary is not None:
        ctx.set_boundary(boundary)
    ctx.upload(pos, vel)
    return ctx


def make_oracle(pos, vel=None, boundary=None, fixed=(0, 0)):
    o = Oracle()
    o.set_fixed_iterations(*fixed)
    if boundary is not None:
        o.set_boundary(boundary)
    o.set_particles(pos, vel)
    return o


class Trio:
    """switch on, switch off and the oracle on one scene, stepped in lock step"""

    def __init__(self, monkeypatch, pos, vel=None, boundary=None, fixed=(0, 0)):
        self.on = make_ctx(monkeypatch, True, pos, vel, boundary, fixed)
        self.off = make_ctx(monkeypatch, False, pos, vel, boundary, fixed)
        self.o = make_oracle(pos, vel, boundary, fixed)
        self.t_on, self.t_off = y.TimeManager(), y.TimeManager()
        self.phase_counts = []  # per step: counters of the switch-on context (before the step, after phase A, after the step)

    def update_neighborhood(self):
        for c in (self.on, self.off, self.o):
            c.update_neighborhood()

    def step(self, what=""):
        """-> the switch-on context's step statistics.  Both contexts take the path on which the device derives dt itself."""
        so = self.o.dfsph_step()
        stats = []
        for ctx, timer in ((self.on, self.t_on), (self.off, self.t_off)):
            c0 = ctx.correction_counts()
            vmax = ctx.step_begin(timer.simulation_step(), timer.law(DIAM))
            c1 = ctx.correction_counts()
            dt_ns = timer.update_simulation_step(DIAM, vmax)
            st = ctx.step_finish(y.duration_as_secs_f32(dt_ns))
            if ctx is self.on:
                self.phase_counts.append((c0, c1, ctx.correction_counts()))
            assert dt_ns == self.o.timer_step_ns(), what
            assert np.float32(vmax) == np.float32(so["vmax"]), (what, vmax, so["vmax"])
            for k in STAT_KEYS:
                assert st[k] == so[k], (what, k, st[k], so[k])
            for k in ("avg_density_error", "avg_divergence"):
                a, b = np.float32(st[k]), np.float32(so[k])
                assert a == b or abs(a - b) <= np.spacing(max(abs(a), abs(b))), (what, k, a, b)
            stats.append(st)
        for k in STAT_KEYS + ("avg_density_error", "avg_divergence"):
            assert stats[0][k] == stats[1][k], (what, k)
        return stats[0]

    def compare(self, what=""):
        o = self.o
        fo, co = o.cells(False)
        for name, ctx in (("on", self.on), ("off", self.off)):
            w = f"{what} switch {name}:"
            d = ctx.download()
            np.testing.assert_array_equal(d["ids"], o.ids(), w + " ids")
            assert_bits_equal(d["pos"], o.positions(), w + " positions")
            assert_bits_equal(d["vel"], o.velocities(), w + " velocities")
            assert_bits_equal(d["density"], o.densities(), w + " densities")
            ss = ctx.download_solver_state()
            assert_bits_equal(ss["kappa"], o.kappa(), w + " kappa")
            assert_bits_equal(ss["stiffness"], o.stiffness(), w + " stiffness")
            f, c = ctx.download_cells(False)
            np.testing.assert_array_equal(c, co, w + " cell indices")
            np.testing.assert_array_equal(f, fo, w + " cell starts")
            assert_same_neighbors(ctx.download_neighbors(), o.neighbors())
        assert self.off.correction_counts() == (0, 0, 0), "SPHX_ZERO_SKIP=0 hands no flags to any correction"


def test_lattice_every_workgroup_skips(monkeypatch):
    """~20 k particles of reset_fluid, still the start lattice: every k is zero, every workgroup of both corrections skips."""
    pos, boundary = dam_break(float(np.sqrt(20000 / 4050)))
    t = Trio(monkeypatch, pos, boundary=boundary)
    for s in range(6):
        st = t.step(f"step {s}")
        assert st["density_iterations"] == 1 and st["divergence_iterations"] == 1
        t.compare(f"step {s}")
    skipped, window, remote = t.on.correction_counts()
    blocks = (len(pos) + 255) // 256
    assert skipped == 6 * 2 * blocks and window == 0 and remote == 0, (skipped, window, remote, blocks)


def test_mixed_skipping_and_walking_workgroups(monkeypatch):
    """The 100 k dam break after 300 device steps: the column has reached the floor, the upper part is still in free fall.  The state
    (positions and velocities) goes to two fresh contexts and to the oracle, then three steps in lock step.  Both loops must hold
    workgroups that skip and workgroups a window flag stops.  The counters do not say which loop a workgroup belongs to, the phases
    of a step do: every density correction queued by phase A (sphx_step_begin_law) is counted before phase B starts, and phase B
    queues further density iterations only when the step needs more of them than the step before — so in a step that does not,
    phase B's counts are the divergence loop's alone."""
    pos, boundary = dam_break(float(np.sqrt(100000 / 4050)))
    run = y.SphxContext()
    run.set_boundary(boundary)
    run.upload(pos)
    timer = y.TimeManager()
    for _ in range(300):
        vmax = run.step_begin(timer.simulation_step(), timer.law(DIAM))
        run.step_finish(y.duration_as_secs_f32(timer.update_simulation_step(DIAM, vmax)))
    d = run.download()
    run.close()
    t = Trio(monkeypatch, d["pos"], d["vel"], boundary)
    prev_iters = 0
    dens = np.zeros(3, np.int64)
    div = np.zeros(3, np.int64)
    div_steps = 0
    for s in range(3):
        st = t.step(f"step {s}")
        t.compare(f"step {s}")
        c0, c1, c2 = (np.array(c, np.int64) for c in t.phase_counts[-1])
        dens += c1 - c0
        if st["density_iterations"] <= max(1, prev_iters):  # phase B queued no density iteration
            div += c2 - c1
            div_steps += 1
        prev_iters = st["density_iterations"]
    print("density loop (skipped, window, remote):", dens, " divergence loop:", div, f"({div_steps} steps)")
    assert dens[0] > 0 and dens[1] > 0, dens
    assert div_steps > 0
    assert div[0] > 0 and div[1] > 0, div


def remote_veto_scene():
    """A sparse lattice (8 neighbours, densities below rho0: every factor zero) over both sides of a high Morton seam — the cell column
    5024 (x = 0.48), where bit 5 of the cell's x index flips: the cells left and right of it are ~2000 sorted slots apart — and, in the
    first cells right of the seam, a 5 x 5 patch at a spacing of 0.003 (24 neighbours, a density far above rho0) inside a hole of
    radius 0.016: the lattice particles left of the seam that still reach the patch keep a density below rho0, so their workgroup's
    window is clear and the patch is known to it only through its out-of-window table.  -> positions, (x0, y0, x1, y1) of the patch."""
    x_seam, y0, psp, gap = 0.48, 0.48, np.float32(0.003), np.float32(0.016)
    nx, ny = int(1.28 / SPACING), int(0.64 / SPACING)
    gx, gy = np.meshgrid(np.arange(nx), np.arange(ny))
    lat = np.stack([np.float32(x_seam - 0.64) + np.float32(0.003) + gx.ravel().astype(np.float32) * SPACING,
                    np.float32(y0) + np.float32(0.003) + gy.ravel().astype(np.float32) * SPACING], -1).astype(np.float32)
    px0, py0 = np.float32(x_seam + 0.0015), np.float32(y0 + 0.0045)
    k = np.arange(5, dtype=np.float32)
    patch = np.stack(np.meshgrid(px0 + k * psp, py0 + k * psp), -1).reshape(-1, 2).astype(np.float32)
    dist = np.sqrt(((lat[:, None, :] - patch[None]) ** 2).sum(-1)).min(1)
    pos = np.concatenate([lat[dist >= gap], patch]).astype(np.float32)
    return pos, (px0 - 1e-4, py0 - 1e-4, px0 + 4 * psp + 1e-4, py0 + 4 * psp + 1e-4)


def test_remote_entry_stops_the_skip(monkeypatch):
    pos, (x0, y0, x1, y1) = remote_veto_scene()
    t = Trio(monkeypatch, pos)
    t.update_neighborhood()
    sp = t.o.positions()
    in_patch = (sp[:, 0] >= x0) & (sp[:, 0] <= x1) & (sp[:, 1] >= y0) & (sp[:, 1] <= y1)
    assert in_patch.sum() == 25
    # the lattice particles that have a patch particle in their list: some of them more than a window (116 slots) away from the patch
    counts, start, lists = t.o.neighbors()
    slots = np.nonzero(in_patch)[0]
    reach = [i for i in range(len(sp)) if not in_patch[i] and np.isin(lists[int(start[i]):int(start[i + 1])], slots).any()]
    assert any(abs(i - int(slots[0])) > 256 + 116 for i in reach), (reach, slots)
    # no wavefront of the scene is in the wide list format (a wavefront turns wide with more than 128 = 512 / 4 entries outside its
    # workgroup's window, sphx_internal.hpp): the third counter, which also counts wide wavefronts, is the remote entries' alone here
    n = len(sp)
    for w0 in range(0, n, 64):
        b0 = (w0 // 256) * 256
        lo, hi = max(0, b0 - 116), min(b0 + 256 + 116, n)
        e = lists[int(start[w0]):int(start[min(w0 + 64, n)])]
        assert np.count_nonzero((e < lo) | (e >= hi)) <= 128, w0
    t.step("step 0")
    # (the oracle keeps kappa by slot: slot i still is the particle that was at sorted slot i when the density loop ran)
    kappa = t.o.kappa()
    assert (kappa[in_patch] != 0).all(), "the patch's factors must be non-zero"
    assert (kappa[~in_patch] == 0).all(), "the lattice's factors must be zero"
    t.compare("step 0")
    skipped, window, remote = t.on.correction_counts()
    assert skipped > 0 and window > 0 and remote > 0, (skipped, window, remote)
    for s in (1, 2):
        t.step(f"step {s}")
        t.compare(f"step {s}")


def line_scene(centre_slot, n=3 * 256 + 1):
    """n particles on one horizontal line inside one row of cells (sorted order = order along x).  All but three sit at the lattice
    spacing (two neighbours, density 70); the three at the sorted slots centre_slot - 1 .. + 1 sit 0.0055 apart, 0.025 away from the
    rest: the middle one's density is 120, i.e. its density factor is the only non-zero k of the scene, its two mates stay at 95."""
    x = np.zeros(n, np.float64)
    pos_x = 0.001
    for i in range(n):
        if i in (centre_slot - 1, centre_slot + 2):
            pos_x += 0.025 - float(SPACING)
        if i in (centre_slot, centre_slot + 1):
            pos_x += 0.0055 - float(SPACING)
        x[i] = pos_x
        pos_x += float(SPACING)
    return np.stack([x.astype(np.float32), np.full(n, 0.51, np.float32)], -1).astype(np.float32)


# (centre slot, workgroups the density correction must see stopped by a window flag).  Workgroup 1's window is [140, 628): flag words
# 2 .. 9 (a word covers 64 slots).  127 is the last slot of word 1, which ends 13 slots below the window: only the owner, workgroup 0,
# may be stopped.  128 is the first slot of word 2, the first word that overlaps the window — the flag is per word, so it must stop
# workgroup 1 as 140, the window's first slot, does.  627 is the window's last slot (word 9, the last one looked at; workgroups 1 and 2).
@pytest.mark.parametrize("centre_slot,stopped", [(127, 1), (128, 2), (256 - 116, 2), (256 + 256 + 116 - 1, 2)])
def test_flag_at_the_edge_of_a_window(monkeypatch, centre_slot, stopped):
    """N = 3 * 256 + 1, one non-zero factor at or next to the first / the last slot of the window of workgroup 1.  One density and one
    divergence iteration: the density correction must see exactly `stopped` workgroups stopped by a window flag and the other
    4 - stopped skip; the divergence correction (fewer than nine neighbours: no factor at all) four skip.
    Sign: a factor of -0 cannot be produced here — the density error is fmax(rho0, .) - rho0 = +0 and the divergence error
    fmax(delta m, 0), whose zero the clamp makes +0, both times a positive alpha; k = +0 is what every skipped workgroup of these
    tests has seen."""
    pos = line_scene(centre_slot)
    t = Trio(monkeypatch, pos, fixed=(1, 1))
    t.update_neighborhood()
    sp = t.o.positions()
    assert np.array_equal(sp[:, 0], pos[:, 0]), "sorted order = order along the line"
    t.step("step 0")
    kappa = t.o.kappa()
    assert kappa[centre_slot] != 0 and np.count_nonzero(kappa) == 1, np.nonzero(kappa)
    t.compare("step 0")
    assert t.on.correction_counts() == (4 - stopped + 4, stopped, 0)


def test_nan_velocity_takes_the_same_course_with_and_without_the_switch(monkeypatch):
    """One NaN velocity in the lattice.  The step does not survive it (the maximum velocity is not finite: SPHX_ERR_NONFINITE, as the
    reference panics), but the first density iteration has run by then — every workgroup of its correction skipping, the counters
    say — and whatever it left must be the same bits with and without the switch."""
    pos, boundary = dam_break(float(np.sqrt(20000 / 4050)))
    vel = np.zeros_like(pos)
    vel[len(pos) // 2, 0] = np.float32("nan")
    out = []
    for skip in (True, False):
        ctx = make_ctx(monkeypatch, skip, pos, vel, boundary)
        timer = y.TimeManager()
        with pytest.raises(y.SphxError) as e:
            ctx.step_begin(timer.simulation_step(), timer.law(DIAM))
        assert e.value.code == y._lib.ERR_NONFINITE
        # The density correction queued behind the prediction HAS run, with a finite dt (the timer law clamps what it derives from the
        # NaN maximum), and with the NaN in its windows: the particle's own error and its neighbours' are fmax(rho0, NaN) - rho0 = 0,
        # so every k is zero and every workgroup of that one launch skips.  (A NaN k itself cannot be made through the interface —
        # the errors are fmax(., .) of a NaN and a number, alpha is finite — so knz_store's "NaN counts" has no scene to test it.)
        assert ctx.correction_counts() == (((len(pos) + 255) // 256, 0, 0) if skip else (0, 0, 0))
        d = ctx.download()
        ss = ctx.download_solver_state()
        out.append((d["pos"], d["vel"], d["density"], d["ids"], ss["kappa"], ss["stiffness"], ss["alpha"]))
    for a, b in zip(*out):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert np.isnan(out[0][1]).any()
