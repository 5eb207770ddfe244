"""Lock-step comparison of a WCSPH implementation with the float64 restatement (tests/dfsph_reference64.py), and the mutants of
the restatement's WCSPH and viscosity routines.

An implementation offers what SphxContext does: upload, clear_cached, wcsph_step_begin(dt) -> vmax, wcsph_step_finish(dt2), download,
download_wcsph_half_step (download between the two phases), download_accel, download_neighbors, download_boundary.  `WcsphRun.step` records one step: the state before it (positions,
velocities, ids, the accelerations it holds), the state between the two phases (positions, v at the half step, Poly6 densities,
ids, accelerations, lists, sorted boundary) and the velocities after it.  `check_step` restates every part of
WCSPHSolver::simulation_step (wscsph.rs:126-179) from the state BEFORE that part, so nothing drifts over steps, and compares within
the bound of tests/dfsph_lockstep.py, |dev - ref| <= C (n + K) 2^-24 M, for every particle:

    leapfrog_position, leapfrog_velocity   leap frog 1 from the state before the step, matched through the ids      K leapfrog, n = 0
    density                                Poly6 densities on the implementation's lists                             K density
    accel                                  update_accellerations on the half-step state                              K wcsph_accel
    vmax_sq                                max |v + a dt|^2 on the restated accelerations                            K vmax_sq, n = max n
    vmax_sq_own                            the same on the implementation's own accelerations                        K wcsph_vmax_sq, n = 0
    velocity                               leap frog 2 on the restated accelerations                                 K wcsph_velocity
    leapfrog2                              leap frog 2 on the implementation's own accelerations                     K leapfrog, n = 0

The two `own` forms are there because the magnitude of the restated accelerations is large next to the accelerations themselves (a
particle at rest density carries the cancellation of a^7 - 1 at a = 1 in every pressure term): a wrong dt in the timer's maximum or in
leap frog 2 changes the result by less than that bound allows, and by far more than the few roundings between an implementation's own
fp32 accelerations and its own result.

Mutants: one plausible misreading of the Rust source each (the docstring names it).  Replaying recorded steps (or, for the
viscosity mutants, recorded DFSPH sub-steps as well) through one must exceed ratio 1.  Not among them, because no scene can tell it
from round-off: the Spiky gradient without its DIVISION_EPSILON (kernel.rs:9, spiky.rs:36) — list members are at least 1e-5 apart
(neighborhood_search.rs:323), so r + 1e-10 differs from r by 1e-5 relative at the very most and by less than one fp32 ulp (6e-8
relative) from r = 1.7e-3 on, below every particle spacing used here; the term's bound is some 50 ulp of its magnitude."""
import numpy as np

from dfsph_lockstep import _by_id, _combined, check_membership
from dfsph_reference64 import KERNEL_POLY6, Restatement, norm

F = np.float32


# ------------------------------------------------------------------------------------------------- the fp32 chain as an implementation
class ChainWcsph:
    """The project's fp32 restatement chain (viscosity_reference.wcsph_* over an Oracle as grid and density provider, the chain
    test_viscosity_host.numpy_wcsph_run proves bit-equal to orc_wcsph_step) behind the interface of SphxContext."""

    def __init__(self, model, coef, params=None, oracle=None):
        from oracle.oracle import Oracle
        from viscosity_reference import Constants

        self.model, self.coef, self.K = model, F(coef), Constants(params)
        self.prov = Oracle() if oracle is None else oracle
        self.acc = np.zeros((0, 2), F)
        self.pos = self.vel = self.ids = self.density = None

    def set_boundary(self, xy):
        self.prov.set_boundary(xy)

    def upload(self, pos, vel=None):
        self.pos = np.array(pos, F).reshape(-1, 2)
        self.vel = np.zeros_like(self.pos) if vel is None else np.array(vel, F).reshape(-1, 2)
        self.ids = np.arange(len(self.pos), dtype=np.uint32)
        self.density = np.zeros(len(self.pos), F)

    def clear_cached(self):
        self.acc = np.zeros((0, 2), F)  # accellerations.clear(), wscsph.rs:123

    @property
    def n(self):
        return len(self.pos)

    def wcsph_step_begin(self, dt):
        from viscosity_reference import wcsph_accel, wcsph_leapfrog1

        dt = F(dt)
        acc = np.zeros((self.n, 2), F)  # accellerations.resize(n, zero), wscsph.rs:128
        k = min(len(self.acc), self.n)
        acc[:k] = self.acc[:k]
        pos, vel = wcsph_leapfrog1(self.pos, self.vel, acc, dt)
        p = self.prov
        p.set_particles(pos, vel)  # (the provider's ids restart at 0..n-1: after the sort they are the permutation)
        p.update_neighborhood()
        p.update_densities(KERNEL_POLY6)
        self.ids = self.ids[p.ids()]
        self.pos, self.vel, self.density = p.positions(), p.velocities(), p.densities()
        self.acc = wcsph_accel(self.model, self.coef, self.K, self.pos, self.vel, self.density, p.boundary(), p.neighbors(), dt)
        w = self.vel + self.acc * dt
        return float(np.sqrt(np.max(w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1], initial=F(0.0))))

    def wcsph_step_finish(self, dt):
        self.vel = self.vel + F(F(0.5) * F(dt)) * self.acc

    def download(self):
        return dict(pos=self.pos.copy(), vel=self.vel.copy(), density=self.density.copy(), ids=self.ids.copy())

    download_wcsph_half_step = download

    def download_accel(self):
        out = np.zeros((self.n, 2), F)
        k = min(len(self.acc), self.n)
        out[:k] = self.acc[:k]
        return out

    def download_neighbors(self):
        return self.prov.neighbors()

    def download_boundary(self):
        return self.prov.boundary(), None

    def close(self):
        pass


# --------------------------------------------------------------------------------------------------------------------- running
class WcsphRun:
    """Drives an implementation step by step with a TimeManager of the app's WCSPH factor (main.rs:116-119) and keeps count of the
    slots the solver's `accellerations` holds (wscsph.rs:122-129), which no implementation is asked for."""

    def __init__(self, impl, diameter=F(0.01), timer=None):
        import yasph2d_amd as y

        self.impl, self.diameter = impl, F(diameter)
        self.timer = y.TimeManager(cfl_factor=0.2) if timer is None else timer
        self.held = 0

    def clear_cached(self):
        self.impl.clear_cached()
        self.held = 0

    def step(self, record=True):
        import yasph2d_amd as y

        impl = self.impl
        dt = float(F(self.timer.simulation_step()))
        rec = dict(dt=dt, held=self.held)
        if record:
            d = impl.download()
            rec["pre"] = dict(pos=d["pos"].copy(), vel=d["vel"].copy(), ids=d["ids"].copy(),
                              accel=impl.download_accel().copy() if self.held else np.zeros((0, 2), F))
        vmax = impl.wcsph_step_begin(dt)
        if record:
            d = impl.download_wcsph_half_step()
            counts, _, lists = impl.download_neighbors()
            rec["mid"] = dict(pos=d["pos"].copy(), vel=d["vel"].copy(), density=d["density"].copy(), ids=d["ids"].copy(),
                              accel=impl.download_accel().copy(), counts=counts, lists=lists, boundary=impl.download_boundary()[0])
        dt2 = float(F(y.duration_as_secs_f32(self.timer.update_simulation_step(self.diameter, vmax))))
        impl.wcsph_step_finish(dt2)
        rec.update(vmax=float(F(vmax)), dt2=dt2)
        self.held = impl.n
        if record:
            d = impl.download()
            rec["post"] = dict(pos=d["pos"].copy(), vel=d["vel"].copy(), density=d["density"].copy(), ids=d["ids"].copy())
        return rec


# -------------------------------------------------------------------------------------------------------------------- checking
def check_step(rec, ref, bounds, where="", rows=None, model=None):
    """One recorded step against `ref` (module docstring).  rows: walk the neighbour lists of these particles (slots of the state
    between the phases) only; what needs no list is still compared for every particle, vmax_sq on the restated accelerations is not
    compared."""
    pre, mid, post = rec["pre"], rec["mid"], rec["post"]
    dt, dt2 = rec["dt"], rec["dt2"]
    n = len(pre["pos"])
    assert len(mid["pos"]) == n == len(post["vel"]), where + ": a step changed the particle count"
    # leap frog 1, wscsph.rs:141-150, and the re-sort of update_neighborhood_datastructure (:153)
    a0 = ref.previous_accellerations(pre["accel"], rec["held"], n)
    x, x_m, v, v_m = ref.leap_frog_1(pre["pos"], pre["vel"], a0, dt)
    perm = _by_id(mid["ids"], pre["ids"])
    bounds.check("leapfrog_position", mid["pos"], x[perm], x_m[perm], 0, "leapfrog", mid["ids"], where)
    bounds.check("leapfrog_velocity", mid["vel"], v[perm], v_m[perm], 0, "leapfrog", mid["ids"], where)
    # update_densities(Poly6), :154, and update_accellerations, :155, on the state the re-sort left
    r = slice(None) if rows is None else rows
    ids = mid["ids"][r]
    X = _combined(mid)
    sl = ref.slots(mid["counts"], mid["lists"], n, rows)
    rho, rho_m = ref.update_densities(X, sl, KERNEL_POLY6)
    bounds.check("density", mid["density"][r], rho, rho_m, sl.n_total, "density", ids, where)
    acc, acc_m = ref.update_accellerations(X, mid["vel"], mid["density"], sl, dt, model)
    bounds.check("accel", mid["accel"][r], acc, acc_m, sl.n_total, "wcsph_accel", ids, where)
    # the timer's maximum, :160-163
    own, own_m = mid["accel"].astype(np.float64), norm(mid["accel"].astype(np.float64))
    vmax_sq = float(F(rec["vmax"])) ** 2
    if rows is None:
        vsq, vsq_m = ref.wcsph_max_velocity_sq(mid["vel"], acc, acc_m, dt)
        bounds.check("vmax_sq", [vmax_sq], [vsq], [vsq_m], [sl.n_total.max(initial=0)], "vmax_sq", None, where)
    vsq, vsq_m = ref.wcsph_max_velocity_sq(mid["vel"], own, own_m, dt)
    bounds.check("vmax_sq_own", [vmax_sq], [vsq], [vsq_m], [0], "wcsph_vmax_sq", None, where)
    # leap frog 2 with the timer's new dt, :164-177
    v2, v2_m = ref.leap_frog_2(mid["vel"][r], acc, acc_m, dt, dt2)
    bounds.check("velocity", post["vel"][r], v2, v2_m, sl.n_total, "wcsph_velocity", ids, where)
    v2, v2_m = ref.leap_frog_2(mid["vel"], own, own_m, dt, dt2)
    bounds.check("leapfrog2", post["vel"], v2, v2_m, 0, "leapfrog", mid["ids"], where)
    for k in ("pos", "density", "ids"):
        assert np.array_equal(post[k].view(np.uint32), mid[k].view(np.uint32)), f"{where}: leap frog 2 changed {k}"
    return bounds


def membership_of_step(rec, h, seed=0, grid_min=(-100.0, -100.0)):
    check_membership(rec["mid"], h, seed=seed, grid_min=grid_min)


def run_and_check(run, steps, ref, bounds, where="", rows=None):
    """`steps` recorded steps, each checked and dropped -> the records' scalars [(dt, dt2, vmax)]."""
    out = []
    for s in range(steps):
        rec = run.step()
        check_step(rec, ref, bounds, f"{where} step {s}", rows)
        out.append((rec["dt"], rec["dt2"], rec["vmax"]))
    return out


# --------------------------------------------------------------------------------------------------------------------- mutants
class MuellerLaplacianNormalizer(Restatement):
    """the viscosity Laplacian normalised as Mueller et al.'s 3D kernel, 45 / (pi h^6), instead of viscosity.rs:24"""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.viscosity_laplacian_norm = 45.0 / (np.pi * self.h ** 6)


class PhysicalOverDt(Restatement):
    """the physical term divided by dt, as the XSPH term is (physical.rs:21 ignores _dt)"""

    def physical_time_scale(self, f, f_m, dt):
        return f / dt, f_m / dt


class ViscousDensityOfI(Restatement):
    """rho_i instead of rho_j in the viscous term"""

    def viscous_density(self, rho, sl, mask):
        return np.broadcast_to(np.asarray(rho, np.float64)[sl.rows][:, None], mask.shape)


class ViscousOverStatic(Restatement):
    """the viscous term over the static neighbours too (v_j = 0, rho_j = rho0)"""

    def viscous_mask(self, sl):
        return sl.valid


class TaitExponent6(Restatement):
    """the Tait equation with exponent 6"""

    def tait_exponent(self):
        return 6


class SpeedOfSoundWithoutSqrt(Restatement):
    """c = v_max / eta instead of v_max / sqrt(eta) (wscsph.rs:47)"""

    def set_compressibility(self, target_density_variation, expected_max_flow_speed):
        super().set_compressibility(target_density_variation ** 2, expected_max_flow_speed)


class PressureTermPerDensitySquared(Restatement):
    """the pressure term as -m (p_i / rho_i^2 + p_j / rho_j^2), the other common symmetric form"""

    def pressure_pair(self, p_i, p_j, rho_i, rho_j):
        return -self.mass * (p_i / (rho_i * rho_i) + p_j / (rho_j * rho_j))


class SpikyGradientFlipped(Restatement):
    """the Spiky gradient with the sign of the analytic derivative, -n_grad (h - r)^2 / r ri_to_rj (spiky.rs:36 has none)"""

    def spiky_gradient_sign(self):
        return -1.0


class BoundaryForceOverR(Restatement):
    """the boundary force as W / r instead of W / r^2 (wscsph.rs:115)"""

    def boundary_force(self, d, r_sq, r):
        return super().boundary_force(d, np.sqrt(r_sq), r)


class BoundaryForceScaled(Restatement):
    """the boundary force factor 1.001 instead of 1"""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.boundary_force_factor = 1.001


class LeapFrog1FullDt(Restatement):
    """leap frog 1 kicking with dt instead of 0.5 dt"""

    def half_kick(self, dt):
        return dt


class LeapFrog2OldDt(Restatement):
    """leap frog 2 with the step's dt instead of the one the timer just returned"""

    def half_kick_2(self, dt, dt_new):
        return 0.5 * dt


class VmaxHalfDt(Restatement):
    """the timer's maximum over |v + a dt / 2| instead of |v + a dt|"""

    def vmax_dt(self, dt):
        return 0.5 * dt


VISCOSITY_MUTANTS = [ViscousDensityOfI, ViscousOverStatic]                      # either model
PHYSICAL_MUTANTS = [MuellerLaplacianNormalizer, PhysicalOverDt]                 # the physical model only
WCSPH_MUTANTS = [TaitExponent6, SpeedOfSoundWithoutSqrt, PressureTermPerDensitySquared, SpikyGradientFlipped, BoundaryForceOverR,
                 BoundaryForceScaled, LeapFrog1FullDt, LeapFrog2OldDt, VmaxHalfDt]
