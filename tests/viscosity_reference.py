"""TEST INFRASTRUCTURE: the reference's viscosity models restated in numpy float32, composed with the oracle's sub-steps.

The oracle (oracle/sph_oracle.cpp) only knows XSPHViscosityModel.  PhysicalViscosityModel (src/sph/viscositymodel/physical.rs:21-23
with the Viscosity kernel's Laplacian, src/sph/smoothing_kernel/viscosity.rs:19-47) is restated here instead, and everything else of a
DFSPH step still runs through the oracle's sub-step entry points (the ones tests/tile_oracle_backend.py drives).

WCSPHSolver::update_accellerations (wscsph.rs:59-118) is restated too (`wcsph_accel`), with either model, and `wcsph_step` chains it
into a whole WCSPH step (leap frog 1, the neighbour lists and Poly6 densities of a provider, the accelerations, vmax, the timer, leap
frog 2) — over the oracle on CPU, over the device's own downloads in the GPU tests.

Exactness rules of the restatement: elementwise IEEE float32 operations only (numpy never fuses a multiply into an add), every
expression in the reference's evaluation order, the per-neighbour sum in list order with one masked np.where per list slot (a masked
lane adds nothing), and np.sqrt for r_sq.sqrt() (correctly rounded, as the device's sqrt_dist is proven to be).
"""
import numpy as np

from tile_oracle_backend import OracleTileBackend
from tiles_reference import in_rect

import yasph2d_amd as y

F = np.float32
PI_F = F(np.pi)
XSPH, PHYSICAL = "xsph", "physical"


def rs_powi(a, b):
    """f32::powi -> compiler-rt __powisf2: square and multiply (b > 0)."""
    a, r = F(a), F(1.0)
    while True:
        if b & 1:
            r = F(r * a)
        b //= 2
        if b == 0:
            return r
        a = F(a * a)


class Constants:
    """The kernel constants the reference derives from the smoothing length (params: a parameter block; default: the reference app's)."""

    def __init__(self, params=None):
        p = y.default_params() if params is None else params
        self.h, self.m, self.rho0 = F(p.smoothing_length), F(p.particle_mass), F(p.fluid_density)
        self.g = np.array(p.gravity, F)
        h = self.h
        self.p6_hsq, self.p6_norm = F(h * h), F(F(4.0) / F(PI_F * rs_powi(h, 8)))                  # poly6.rs:16-23
        self.vis_nlap = F(F(360.0) / F(F(F(29.0) * PI_F) * rs_powi(h, 5)))                        # viscosity.rs:24
        self.sp_norm = F(F(10.0) / F(PI_F * rs_powi(h, 5)))                                       # spiky.rs:16-23
        self.sp_ngrad = F(F(30.0) / F(PI_F * rs_powi(h, 5)))
        c = F(F(1.0) / np.sqrt(F(0.01)))                                                           # wscsph.rs:31-49
        self.wc_stiffness = F(F(F(self.rho0 * c) * c) / F(7.0))
        self.wc_boundary_force = F(1.0)


def _slots(counts, start, lists, static=False):
    """Per list slot k of the dynamic (static: boundary) neighbours: (mask of the particles that have a k-th entry, its index)."""
    cd = counts[:, 0].astype(np.int64)
    cnt = counts[:, 1].astype(np.int64) - cd if static else cd
    st = start[:-1].astype(np.int64) + (cd if static else 0)
    top = max(len(lists) - 1, 0)
    for k in range(int(cnt.max()) if len(cnt) else 0):
        m = cnt > k
        j = np.where(m, lists[np.minimum(st + k, top)] if len(lists) else 0, 0).astype(np.int64)
        yield m, j


def viscous_term(model, coef, K, dt, r_sq, r, rho_j):
    """compute_viscous_accelleration without the velocity difference: the scalar it is multiplied with."""
    if model == PHYSICAL:  # fluid_viscosity * massj * laplacian(r_sq, r) / rhoj, physical.rs:22; laplacian = nlap * (h - r), viscosity.rs:45
        return F(F(F(coef) * K.m) * F(K.vis_nlap * F(K.h - r))) / rho_j
    dsq = np.maximum(F(K.p6_hsq - r_sq), F(0.0))  # XSPH: epsilon * massj * Poly6::evaluate / (rhoj * dt), xsph.rs:22
    w = F(F(F(K.p6_norm * dsq) * dsq) * dsq)
    return F(F(F(coef) * K.m) * w) / F(rho_j * F(dt))


def nonpressure_accel(model, coef, K, pos, vel, rho, nb, dt):
    """dfsph.rs:436-469 for every particle of the set: gravity * m / m plus the viscous term of each dynamic neighbour, in list order."""
    n = len(pos)
    a0 = (K.g * K.m) / K.m
    ax, ay = np.full(n, a0[0], F), np.full(n, a0[1], F)
    for m, j in _slots(*nb):
        dx, dy = pos[j, 0] - pos[:, 0], pos[j, 1] - pos[:, 1]
        r_sq = dx * dx + dy * dy
        f = viscous_term(model, coef, K, dt, r_sq, np.sqrt(r_sq), rho[j])
        ax = np.where(m, ax + f * (vel[j, 0] - vel[:, 0]), ax)
        ay = np.where(m, ay + f * (vel[j, 1] - vel[:, 1]), ay)
    return np.stack([ax, ay], 1)


def wcsph_pressure(K, rho):
    """Tait equation with clamping (wscsph.rs:52-57); powi(7) in compiler-rt's order."""
    a = np.maximum(rho / K.rho0, F(1.0))
    r = a
    a = a * a
    r = r * a
    a = a * a
    return K.wc_stiffness * (r * a - F(1.0))


def wcsph_accel(model, coef, K, pos, vel, rho, boundary, nb, dt):
    """WCSPHSolver::update_accellerations (wscsph.rs:59-118): gravity; per dynamic neighbour the pressure term (Spiky gradient) and then
    the viscous term; per static neighbour the boundary force (wscsph.rs:109-116).  Static list entries index `boundary`."""
    n = len(pos)
    dt = F(dt)
    pi = wcsph_pressure(K, rho)
    ax, ay = np.full(n, K.g[0], F), np.full(n, K.g[1], F)
    for m, j in _slots(*nb):
        dx, dy = pos[j, 0] - pos[:, 0], pos[j, 1] - pos[:, 1]  # ri_to_rj
        r_sq = dx * dx + dy * dy
        r = np.sqrt(r_sq)
        rho_j = rho[j]
        pu = (-K.m * (pi + wcsph_pressure(K, rho_j))) / ((F(2.0) * rho) * rho_j)   # wscsph.rs:99
        d = np.maximum(K.h - r, F(0.0))
        sg = ((K.sp_ngrad * d) * d) / (r + F(1.0e-10))                             # Spiky::gradient, spiky.rs:34-37
        tx, ty = ax + pu * (sg * dx), ay + pu * (sg * dy)
        f = viscous_term(model, coef, K, dt, r_sq, r, rho_j)
        ax = np.where(m, tx + f * (vel[j, 0] - vel[:, 0]), ax)
        ay = np.where(m, ty + f * (vel[j, 1] - vel[:, 1]), ay)
    for m, j in _slots(*nb, static=True):
        q = boundary[j]
        dx, dy = q[:, 0] - pos[:, 0], q[:, 1] - pos[:, 1]
        r_sq = dx * dx + dy * dy
        d = np.maximum(K.h - np.sqrt(r_sq), F(0.0))
        s = (K.wc_boundary_force * (((K.sp_norm * d) * d) * d)) / r_sq              # Spiky::evaluate / r_sq, wscsph.rs:114
        s = np.where(m, s, F(0.0))  # (masked lanes may divide 0 by 0)
        ax = np.where(m, ax - s * dx, ax)
        ay = np.where(m, ay - s * dy, ay)
    return np.stack([ax, ay], 1)


def wcsph_leapfrog1(pos, vel, acc, dt):
    """wscsph.rs:138-149: v += (0.5 dt) a, x += v dt."""
    vel = vel + F(F(0.5) * F(dt)) * acc
    return pos + vel * F(dt), vel


def wcsph_finish(model, coef, K, pos, vel_half, rho, boundary, nb, dt, timer, diameter):
    """The rest of WCSPHSolver::simulation_step after the density update (wscsph.rs:154-177) on the state a provider re-gridded:
    -> (accelerations, vmax, dt_ns of the timer, final velocities)."""
    import yasph2d_amd as yy

    acc = wcsph_accel(model, coef, K, pos, vel_half, rho, boundary, nb, dt)
    p = vel_half + acc * F(dt)
    vmax = np.sqrt(np.max(p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1], initial=F(0.0)))
    dt_ns = timer.update_simulation_step(diameter, vmax)
    dt2 = F(yy.duration_as_secs_f32(dt_ns))
    return acc, F(vmax), dt_ns, vel_half + F(F(0.5) * dt2) * acc


class ViscousOracleTileBackend(OracleTileBackend):
    """OracleTileBackend with the non-pressure pass and the velocity prediction in numpy: model "xsph" (coef = epsilon) or
    "physical" (coef = fluid_viscosity).  The oracle keeps positions, lists, densities and everything after the prediction."""

    def __init__(self, model, coef, params=None, oracle=None):
        """params, oracle: a parameter block and an Oracle made with the same constants (default: the reference app's)."""
        if params is None:
            super().__init__(oracle)
        else:
            super().__init__(oracle, h=params.smoothing_length, grid_min=tuple(params.grid_min))
        assert model in (XSPH, PHYSICAL)
        self.model, self.coef, self.K = model, F(coef), Constants(params)

    def nonpressure(self, dt_prev):
        pos, vel, ids, _, _ = self._state()
        if len(pos) == 0:
            self.accel = np.zeros((0, 2), F)
            return 0.0
        rho = self.o.densities()
        counts, start, lists = self.o.neighbors()
        self.accel = nonpressure_accel(self.model, self.coef, self.K, pos, vel, rho, (counts, start, lists), F(dt_prev))
        p = vel + self.accel * F(dt_prev)
        vsq = p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]
        cx, cy = self._cells(pos)
        owned = in_rect(cx, cy, self.rect)  # tile_owns: the cell of the position lies in the tile rectangle (orc_sub_nonpressure)
        return float(np.max(vsq[owned], initial=F(0.0)))

    def predict(self, dt):
        """v + a dt (dfsph.rs:484-492), written back with the state the oracle holds; the re-grid of unmoved positions returns the same
        order, lists, densities and alpha."""
        pos, vel, ids, kappa, stiff = self._state()
        vel = vel + self.accel * F(dt)
        self._set(pos, vel, ids, kappa, stiff)
        self.L.orc_sub_regrid(self.o.h)


