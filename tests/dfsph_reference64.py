"""A float64 restatement of the reference DFSPH and WCSPH steps and of both viscosity models, written from the yasph2d Rust
sources alone.

Every function below names the lines of the reference it restates (paths relative to yasph2d's `src/sph/`).  It is plain numpy in
float64 and shares no code with the oracle or the HIP kernels: the inputs are the fp32 state of an implementation (positions,
velocities, densities, alpha, warm-start values, neighbour lists), the outputs are what one reference routine makes of them.

Next to each output every function returns a float64 magnitude M: the same expression with every term replaced by its absolute
value, and every subtraction that may cancel counted at the size of its operands (v_i - v_j as |v_i| + |v_j|, rho + delta m dt -
rho0 as rho + |delta| m dt + rho0).  In a kernel's power of a cancelling difference, d^k with d = 1 - q, h^2 - r^2 or h - r, the
operand size enters to first order: k d^(k-1) |dq| is the rounding of d^k when q carries a relative error, so its magnitude is
(d + 8u s)^(k-1) (d + k s), s the operand size (q, h^2 + r^2, h + r), u = 2^-24 (the 8u keeps a pair at q = 1 from demanding an
exact zero).  An fp32 evaluation of the expression in any order then lies within a few units of 2^-24 M per term of its sum;
`tests/dfsph_lockstep.py` turns that into the bound it asserts.

Only these inputs are taken from the library's parameters: the smoothing length, the fluid density, the particle density, gravity
and the viscosity model with its coefficient (all fp32).  The kernel normalisers (Wendland, Poly6, Spiky and its gradient, the
viscosity kernel's Laplacian), the particle mass, the radius, the WCSPH stiffness and its boundary force factor are derived here in
float64 from the Rust formulas, so a wrong constant in an implementation shows up as a mismatch.
"""
import numpy as np

# dfsph.rs:49,53 (relative density deviation per second)
MAX_AVG_DENSITY_ERROR = 0.01 / 100.0
MAX_DIVERGENCE_ERROR = 0.1 / 100.0
ALPHA_EPSILON = 1e-6          # dfsph.rs:70
MIN_NEIGHBORS = 9             # dfsph.rs:261, "particle deficiency"
MIN_DISTANCE_SQ = 1.0e-10     # neighborhood_search.rs:323
MAX_NUM_NEIGHBORS = 64        # neighborhood_search.rs:322
XSPH_EPSILON = 0.05           # viscositymodel/xsph.rs:14
FLUID_VISCOSITY = 1.0016 / 1000.0  # viscositymodel/physical.rs:14
DIVISION_EPSILON = 1.0e-10    # smoothing_kernel/kernel.rs:9
TAIT_EQUATION_GAMMA = 7       # solver/wscsph.rs:26
XSPH, PHYSICAL = "xsph", "physical"

KERNEL_WENDLAND, KERNEL_POLY6, KERNEL_SPIKY = 0, 1, 2
U = 2.0 ** -24


def power_of_difference(d, size, k):
    """d^k for a difference d >= 0 of operands of size `size`, and its magnitude (module docstring)."""
    return d ** k, (d + 8 * U * size) ** (k - 1) * (d + k * size)


def f64(a):
    return np.asarray(a, dtype=np.float64)


def norm(v):
    return np.sqrt((v * v).sum(-1))


class Slots:
    """Neighbour lists of the particles `rows` as (R, S) slot matrices.

    Input in the canonical form: counts[N, 2] = (dynamic, total) and the flat list of every particle's entries, dynamic ones first
    (fluid indices), then static ones (boundary indices).  `j` addresses the combined array [fluid | boundary] (a static entry b
    becomes n_fluid + b); `valid`, `dyn` and `stat` mask the slots.  `drop` leaves out the last `drop` entries of every list."""

    def __init__(self, counts, lists, n_fluid, rows=None, drop=0):
        counts = np.asarray(counts)
        n_dyn_all, n_tot_all = counts[:, 0].astype(np.int64), counts[:, 1].astype(np.int64)
        start_all = np.zeros(len(counts) + 1, np.int64)
        np.cumsum(n_tot_all, out=start_all[1:])
        self.rows = np.arange(len(counts)) if rows is None else np.asarray(rows, np.int64)
        n_dyn, n_tot = n_dyn_all[self.rows], n_tot_all[self.rows]
        if drop:
            n_tot = np.maximum(n_tot - drop, 0)
            n_dyn = np.minimum(n_dyn, n_tot)
        width = max(1, int(n_tot.max()) if len(n_tot) else 1)
        s = np.arange(width)[None, :]
        self.valid = s < n_tot[:, None]
        self.dyn = s < n_dyn[:, None]
        self.stat = self.valid & ~self.dyn
        flat = np.asarray(lists)
        idx = np.where(self.valid, start_all[self.rows][:, None] + s, 0)
        j = flat[idx].astype(np.int64) if len(flat) else np.zeros(idx.shape, np.int64)
        self.j = np.where(self.stat, n_fluid + j, np.where(self.dyn, j, 0))
        self.n_total = n_tot
        self.n_fluid = n_fluid


class Restatement:
    """The reference DFSPHSolver / WCSPHSolver<XSPHViscosityModel | PhysicalViscosityModel> + FluidParticleWorld routines, one
    method per routine.  model: ("xsph", epsilon) or ("physical", mu)."""

    def __init__(self, smoothing_length, fluid_density, particle_density, gravity, model=(XSPH, XSPH_EPSILON)):
        assert model[0] in (XSPH, PHYSICAL), model
        self.model = (model[0], float(np.float32(model[1])))
        self.h = float(np.float32(smoothing_length))
        self.rho0 = float(np.float32(fluid_density))
        self.particle_density = float(np.float32(particle_density))
        self.gravity = f64(np.asarray(gravity, np.float32))
        # fluidparticleworld.rs:74-76, :83-89
        self.mass = self.rho0 / self.particle_density
        self.radius = 0.5 / np.sqrt(self.particle_density)
        h = self.h
        # smoothing_kernel/wendland_quintic_c2.rs:23-30, poly6.rs:14-20, spiky.rs:14-20
        self.wendland_norm = 4.0 * 7.0 / (np.pi * h ** 2)
        self.wendland_grad_norm = 140.0 / (np.pi * h ** 4)
        self.poly6_norm = 4.0 / (np.pi * h ** 8)
        self.spiky_norm = 10.0 / (np.pi * h ** 5)
        self.spiky_grad_norm = 30.0 / (np.pi * h ** 5)           # spiky.rs:21
        self.viscosity_laplacian_norm = 360.0 / (29.0 * np.pi * h ** 5)  # viscosity.rs:24
        # solver/wscsph.rs:34,39,47-48: new() calls set_compressibility(eta = 0.01, expected max flow speed 1)
        self.boundary_force_factor = 1.0
        self.set_compressibility(0.01, 1.0)

    def set_compressibility(self, target_density_variation, expected_max_flow_speed):
        """wscsph.rs:45-49: c = v_max / sqrt(eta), B = rho0 c c / gamma."""
        self.speed_of_sound = expected_max_flow_speed / np.sqrt(target_density_variation)
        self.stiffness = self.rho0 * self.speed_of_sound * self.speed_of_sound / TAIT_EQUATION_GAMMA

    @classmethod
    def from_params(cls, params, particle_density):
        """params: the library's parameter block (smoothing_length, fluid_density, gravity, viscosity_model, fluid_viscosity,
        xsph_epsilon); particle_density: the value it was made with (the block does not carry it)."""
        model = (PHYSICAL, params.fluid_viscosity) if int(params.viscosity_model) == 1 else (XSPH, params.xsph_epsilon)
        return cls(params.smoothing_length, params.fluid_density, particle_density, tuple(params.gravity), model)

    # ---- neighbour lists -------------------------------------------------------------------------------------------------------
    def slots(self, counts, lists, n_fluid, rows=None):
        return Slots(counts, lists, n_fluid, rows)

    # ---- kernels -----------------------------------------------------------------------------------------------------------------
    def wendland_evaluate(self, r):
        """wendland_quintic_c2.rs:33-38: W = n (1 - q)^4 (q + 1/4), q = min(r / h, 1)."""
        q = np.minimum(r / self.h, 1.0)
        p, p_m = power_of_difference(1.0 - q, q, 4)
        return self.wendland_norm * p * (q + 0.25), self.wendland_norm * p_m * (q + 0.25)

    def grad_shape(self, q):
        """(1 - q)^3 of the Wendland gradient and its magnitude."""
        return power_of_difference(1.0 - q, q, 3)

    def wendland_gradient(self, ri_to_rj, r):
        """wendland_quintic_c2.rs:40-46 via kernel.rs:23-28 (gradient_from_positions: ri_to_rj = rj - ri):
        n_grad (1 - q)^3 ri_to_rj, q = min(r / h, 1)."""
        q = np.minimum(r / self.h, 1.0)
        shape, shape_m = self.grad_shape(q)
        return (self.wendland_grad_norm * shape)[..., None] * ri_to_rj, self.wendland_grad_norm * shape_m * r

    def poly6_evaluate(self, r_sq):
        """poly6.rs:24-28: n max(h^2 - r^2, 0)^3."""
        hsq = self.h * self.h
        p, p_m = power_of_difference(np.maximum(hsq - r_sq, 0.0), hsq + r_sq, 3)
        return self.poly6_norm * p, self.poly6_norm * p_m

    def spiky_evaluate(self, r):
        """spiky.rs:24-28: n max(h - r, 0)^3."""
        p, p_m = power_of_difference(np.maximum(self.h - r, 0.0), self.h + r, 3)
        return self.spiky_norm * p, self.spiky_norm * p_m

    def spiky_gradient(self, ri_to_rj, r):
        """spiky.rs:34-37 with kernel.rs:9: n_grad max(h - r, 0)^2 / (r + 1e-10) ri_to_rj."""
        p, p_m = power_of_difference(np.maximum(self.h - r, 0.0), self.h + r, 2)
        s = self.spiky_grad_norm / self.divided_distance(r)
        return (s * p)[..., None] * ri_to_rj * self.spiky_gradient_sign(), s * p_m * r

    def divided_distance(self, r):
        """The divisor of the Spiky gradient (spiky.rs:36): r + DIVISION_EPSILON."""
        return r + DIVISION_EPSILON

    def spiky_gradient_sign(self):
        """+1: the gradient points along ri_to_rj as spiky.rs:36 writes it (no minus sign; the solver's is in wscsph.rs:100)."""
        return 1.0

    def viscosity_laplacian(self, r):
        """viscosity.rs:45-47: n_lap (h - r), with no test of r < h: slightly negative for a list member whose float64 distance
        lies beyond h."""
        d, d_m = power_of_difference(self.h - r, self.h + r, 1)
        return self.viscosity_laplacian_norm * d, self.viscosity_laplacian_norm * d_m

    def evaluate(self, kind, r_sq, r):
        if kind == KERNEL_WENDLAND:
            return self.wendland_evaluate(r)
        if kind == KERNEL_POLY6:
            return self.poly6_evaluate(r_sq)
        if kind == KERNEL_SPIKY:
            return self.spiky_evaluate(r)
        raise ValueError(kind)

    # ---- pair geometry -----------------------------------------------------------------------------------------------------------
    def pair_vectors(self, X, sl):
        """rj - ri, |rj - ri|^2, |rj - ri| for every slot (zero in unused slots)."""
        X = f64(X)
        d = (X[sl.j] - X[sl.rows][:, None, :]) * sl.valid[..., None]
        r_sq = (d * d).sum(-1)
        return d, r_sq, np.sqrt(r_sq)

    def pair_gradients(self, X, sl):
        """Wendland gradient_from_positions(ri, rj) per slot, and its magnitude."""
        d, _, r = self.pair_vectors(X, sl)
        g, m = self.wendland_gradient(d, r)
        return g * sl.valid[..., None], m * sl.valid

    def pair_kernel(self, X, sl, kind):
        _, r_sq, r = self.pair_vectors(X, sl)
        w, m = self.evaluate(kind, r_sq, r)
        return w * sl.valid, m * sl.valid

    # ---- FluidParticleWorld::update_densities ------------------------------------------------------------------------------------
    def update_densities(self, X, sl, kind=KERNEL_WENDLAND):
        """fluidparticleworld.rs:197-231: rho_i = max(rho0, m W(0) + sum_dyn m W(r_ij) + sum_static m W(r_ij))."""
        w0, w0_m = self.evaluate(kind, np.zeros(1), np.zeros(1))
        w, w_m = self.pair_kernel(X, sl, kind)
        rho = self.mass * (w0[0] + w.sum(1))
        return np.maximum(rho, self.rho0), self.mass * (w0_m[0] + w_m.sum(1))

    # ---- DFSPHSolver -------------------------------------------------------------------------------------------------------------
    def compute_alpha_factors(self, X, sl):
        """dfsph.rs:68-97: alpha_i = 1 / max(|sum m grad W_ij|^2 + sum |m grad W_ij|^2, 1e-6) over dynamic and static neighbours."""
        g, g_m = self.pair_gradients(X, sl)
        g, g_m = g * self.mass, g_m * self.mass
        total = g.sum(1)
        denom = (total * total).sum(-1) + (g * g).sum((1, 2))
        denom_m = g_m.sum(1) ** 2 + (g_m * g_m).sum(1)
        dc = np.maximum(denom, ALPHA_EPSILON)
        alpha = 1.0 / dc
        return alpha, denom_m / (dc * dc) + alpha

    def viscous_factor(self, model, X, rho, sl, dt, mask):
        """compute_viscous_accelleration without its velocity difference, per slot of `mask`, and its magnitude.
        xsph.rs:21-23: epsilon m W_poly6(r^2) / (rho_j dt); physical.rs:21-23: mu m laplacian(r) / rho_j, no dt."""
        kind, coef = model
        _, r_sq, r = self.pair_vectors(X, sl)
        rho_j = self.viscous_density(rho, sl, mask)
        if kind == PHYSICAL:
            w, w_m = self.viscosity_laplacian(r)
            f, f_m = coef * self.mass * w / rho_j, abs(coef) * self.mass * w_m / rho_j
            f, f_m = self.physical_time_scale(f, f_m, dt)
        else:
            w, w_m = self.poly6_evaluate(r_sq)
            f, f_m = coef * self.mass * w / (rho_j * dt), abs(coef) * self.mass * w_m / (rho_j * dt)
        return f * mask, f_m * mask

    def viscous_density(self, rho, sl, mask):
        """rhoj of compute_viscous_accelleration: the NEIGHBOUR's density (dfsph.rs:457-466, wscsph.rs:103-105)."""
        return np.where(mask, f64(rho)[np.where(mask, sl.j, 0)], 1.0)

    def physical_time_scale(self, f, f_m, dt):
        """physical.rs:21: `_dt` is unused."""
        return f, f_m

    def viscous_mask(self, sl):
        """The viscosity loops visit neighbors_dynamic only (dfsph.rs:449, wscsph.rs:89)."""
        return sl.dyn

    def viscous_sum(self, model, X, V, rho, sl, dt):
        """sum over the visited neighbours of factor (v_j - v_i); a static neighbour (only a mutant visits one) has v_j = 0."""
        V = f64(V)
        mask = self.viscous_mask(sl)
        if not np.array_equal(mask, sl.dyn):  # a mutant's static visit: boundary particles carry no density; rho0 stands in
            rho = np.concatenate([f64(rho), np.full(len(X) - len(rho), self.rho0)])
            V = np.concatenate([V, np.zeros((len(X) - len(V), 2))])
        f, f_m = self.viscous_factor(model, X, rho, sl, dt, mask)
        vi = V[sl.rows]
        vj = V[np.where(mask, sl.j, 0)]
        return (f[..., None] * (vj - vi[:, None, :])).sum(1), (f_m * (norm(vj) + norm(vi)[:, None])).sum(1)

    def nonpressure(self, X, V, rho, sl, dt_prev, model=None):
        """dfsph.rs:436-469 with xsph.rs:21-23 or physical.rs:21-23: a_i = g + sum_dyn factor_ij (v_j - v_i); the viscosity loop
        visits the dynamic neighbours only, and the model is called with the step length of the previous step.
        model: ("xsph", epsilon) or ("physical", mu); None: the one the restatement was made with."""
        a, a_m = self.viscous_sum(self.model if model is None else model, X, V, rho, sl, dt_prev)
        return self.gravity + a, norm(self.gravity) + a_m

    def max_velocity_sq(self, V, acc, acc_m, dt_prev):
        """dfsph.rs:474-477: max |v + a dt_prev|^2 (the viscosity pass ran with dt_prev, so does this)."""
        w = f64(V) + acc * dt_prev
        m = (norm(f64(V)) + acc_m * dt_prev) ** 2
        return float((w * w).sum(-1).max(initial=0.0)), float(m.max(initial=0.0))

    def predict(self, V, acc, acc_m, dt):
        """dfsph.rs:484-492: v* = v + a dt."""
        return f64(V) + acc * dt, norm(f64(V)) + acc_m * dt

    def _velocity_difference_dot(self, X, V, sl):
        """sum over slots of (v_i - v_j) . grad W_ij, a static neighbour contributing v_i . grad W_ij (dfsph.rs:111-120, :267-276)."""
        V = f64(V)
        g, g_m = self.pair_gradients(X, sl)
        vc = np.concatenate([V, np.zeros((len(X) - len(V), 2))])
        vi = V[sl.rows]
        vj = vc[sl.j] * sl.dyn[..., None]
        dv = vi[:, None, :] - vj
        delta = (dv * g).sum((1, 2))
        delta_m = ((norm(vi)[:, None] + norm(vj)) * g_m).sum(1)
        return delta, delta_m

    def compute_density_error(self, X, V, rho, sl, dt):
        """dfsph.rs:99-126: e_i = max(rho0, rho_i + delta_i m dt) - rho0."""
        delta, delta_m = self._velocity_difference_dot(X, V, sl)
        rho_i = f64(rho)[sl.rows]
        e = np.maximum(self.rho0, rho_i + delta * self.mass * dt) - self.rho0
        return e, rho_i + delta_m * self.mass * dt + self.rho0

    def deficient(self, n_total):
        """dfsph.rs:260-264: fewer than 9 neighbours in all (num_total_neighbors)."""
        return n_total < MIN_NEIGHBORS

    def compute_density_change(self, X, V, sl):
        """dfsph.rs:249-280: c_i = max(0, m sum (v_i - v_j) . grad W_ij), 0 for a particle with fewer than 9 neighbours."""
        delta, delta_m = self._velocity_difference_dot(X, V, sl)
        gate = self.deficient(sl.n_total)
        c = np.where(gate, 0.0, np.maximum(delta * self.mass, 0.0))
        return c, np.where(gate, 0.0, delta_m * self.mass)

    def correct_velocity(self, X, V, k, k_m, sl, scale):
        """The common form of dfsph.rs:128-161, :163-193, :282-314 and :316-344:
        v_i -= scale m (sum_dyn (k_i + k_j) grad W_ij + sum_static k_i grad W_ij); scale = 1/dt in the density loop, 1 in the
        divergence loop.  k: the per-particle stiffness of ALL fluid particles (k_j is read for neighbours)."""
        V, k, k_m = f64(V), f64(k), f64(k_m)
        g, g_m = self.pair_gradients(X, sl)
        kj = np.where(sl.dyn, k[np.where(sl.dyn, sl.j, 0)], 0.0)
        kj_m = np.where(sl.dyn, k_m[np.where(sl.dyn, sl.j, 0)], 0.0)
        ki, ki_m = k[sl.rows], k_m[sl.rows]
        delta = ((ki[:, None] + kj)[..., None] * g).sum(1)
        delta_m = ((ki_m[:, None] + kj_m) * g_m).sum(1)
        vi = V[sl.rows]
        return vi - scale * delta * self.mass, norm(vi) + scale * delta_m * self.mass

    def density_iteration_k(self, X, V, rho, alpha, sl, dt):
        """dfsph.rs:141: k_i = e_i alpha_i (what correct_velocity_with_density_error adds to warmstart_kappa)."""
        e, e_m = self.compute_density_error(X, V, rho, sl, dt)
        a = f64(alpha)[sl.rows]
        return e * a, e_m * a, e, e_m

    def divergence_iteration_k(self, X, V, alpha, sl):
        """dfsph.rs:295: k_i = c_i alpha_i (added to warmstart_stiffness)."""
        c, c_m = self.compute_density_change(X, V, sl)
        a = f64(alpha)[sl.rows]
        return c * a, c_m * a, c, c_m

    def damp(self, k):
        """dfsph.rs:201-203 / :356-358: k = 0.5 max(k, -0.5 rho0^2) before a warm start."""
        return 0.5 * np.maximum(f64(k), -0.5 * self.rho0 * self.rho0)

    def warm_start(self, X, V, k, sl, dt, divergence):
        """dfsph.rs:163-193 (1/dt) and :316-344 (no dt) with the damped warm-start values; -> (v, M, damped k)."""
        kd = self.damp(k)
        v, m = self.correct_velocity(X, V, kd, np.abs(kd), sl, 1.0 if divergence else 1.0 / dt)
        return v, m, kd

    def advect(self, X, V, dt):
        """dfsph.rs:499-510: x += v* dt."""
        return f64(X) + f64(V) * dt, norm(f64(X)) + norm(f64(V)) * dt

    # ---- WCSPHSolver -------------------------------------------------------------------------------------------------------------
    def tait_exponent(self):
        return TAIT_EQUATION_GAMMA

    def pressure(self, rho):
        """wscsph.rs:52-57: B (max(rho / rho0, 1)^7 - 1).  Magnitude: a^7 is seven factors that each carry a's relative error, and
        the subtraction of 1 cancels at a = 1: B (7 a^7 + 1)."""
        g = self.tait_exponent()
        a = np.maximum(f64(rho) / self.rho0, 1.0) ** g
        return self.stiffness * (a - 1.0), self.stiffness * (g * a + 1.0)

    def pressure_pair(self, p_i, p_j, rho_i, rho_j):
        """wscsph.rs:100: -m (p_i + p_j) / (2 rho_i rho_j) (linear in the pressures: the magnitudes go through the same form)."""
        return -self.mass * (p_i + p_j) / (2.0 * rho_i * rho_j)

    def boundary_force(self, d, r_sq, r):
        """wscsph.rs:112-116: per static neighbour -f_b W_spiky(r) / r^2 ri_to_rj -> (vector, magnitude)."""
        w, w_m = self.spiky_evaluate(r)
        rs = np.where(r_sq > 0, r_sq, 1.0)
        return -(self.boundary_force_factor * w / rs)[..., None] * d, self.boundary_force_factor * w_m / rs * r

    def update_accellerations(self, X, V, rho, sl, dt, model=None):
        """wscsph.rs:59-118: a_i = g + sum_dyn (-m (p_i + p_j) / (2 rho_i rho_j) grad W_spiky(ri_to_rj) + viscous term with this
        step's dt) + sum_static (-f_b W_spiky(r) / r^2 ri_to_rj)."""
        rho = f64(rho)
        d, r_sq, r = self.pair_vectors(X, sl)
        p, p_m = self.pressure(rho)
        jd = np.where(sl.dyn, sl.j, 0)
        rho_i = rho[sl.rows][:, None]
        pu = self.pressure_pair(p[sl.rows][:, None], p[jd], rho_i, rho[jd]) * sl.dyn
        pu_m = -self.pressure_pair(p_m[sl.rows][:, None], p_m[jd], rho_i, rho[jd]) * sl.dyn
        g, g_m = self.spiky_gradient(d, r)
        acc = (pu[..., None] * g).sum(1)
        acc_m = (np.abs(pu_m) * g_m).sum(1)
        a, a_m = self.viscous_sum(self.model if model is None else model, X, V, rho, sl, dt)
        b, b_m = self.boundary_force(d, r_sq, r)
        acc = self.gravity + acc + a + (b * sl.stat[..., None]).sum(1)
        acc_m = norm(self.gravity) + acc_m + a_m + (b_m * sl.stat).sum(1)
        return acc, acc_m

    def leap_frog_1(self, X, V, A, dt):
        """wscsph.rs:141-150: v += 0.5 dt a; x += v dt (a: the previous step's accelerations, slot by slot).
        -> (x, M, v, M)"""
        X, V, A = f64(X), f64(V), f64(A)
        v, v_m = V + self.half_kick(dt) * A, norm(V) + self.half_kick(dt) * norm(A)
        return X + v * dt, norm(X) + v_m * dt, v, v_m

    def half_kick(self, dt):
        return 0.5 * dt

    def previous_accellerations(self, accel, n_held, n):
        """wscsph.rs:122-124, :128: `accellerations` is slot-bound; clear_cached_data empties it, resize(n, zero) cuts it to n
        slots or fills up with zeros.  accel: what an implementation holds; n_held: how many slots of it the solver held."""
        out = np.zeros((n, 2))
        k = min(n_held, n)
        out[:k] = f64(accel).reshape(-1, 2)[:k]
        return out

    def wcsph_max_velocity_sq(self, V, acc, acc_m, dt):
        """wscsph.rs:160-163: max |v + a dt|^2 with the step's own dt (before the timer changes it)."""
        return self.max_velocity_sq(V, acc, acc_m, self.vmax_dt(dt))

    def vmax_dt(self, dt):
        return dt

    def leap_frog_2(self, V, acc, acc_m, dt, dt_new):
        """wscsph.rs:164-177: v += 0.5 dt a with the dt the timer just returned."""
        k = self.half_kick_2(dt, dt_new)
        return f64(V) + k * acc, norm(f64(V)) + k * acc_m

    def half_kick_2(self, dt, dt_new):
        return 0.5 * dt_new

    # ---- loop control ------------------------------------------------------------------------------------------------------------
    def average_density_error(self, e):
        """dfsph.rs:221: sum e / N."""
        return float(np.sum(e)) / len(e)

    def average_divergence(self, c):
        """dfsph.rs:376-377: sum c / N / rho0."""
        return float(np.sum(c)) / len(c) / self.rho0

    def density_converged(self, avg, dt):
        """dfsph.rs:222,226: avg / rho0 * dt < max_avg_density_error."""
        return avg / self.rho0 * dt < MAX_AVG_DENSITY_ERROR

    def divergence_converged(self, avg, dt):
        """dfsph.rs:381: avg * dt < max_divergence_error."""
        return avg * dt < MAX_DIVERGENCE_ERROR


def brute_force_neighbors(pos, boundary, h, i):
    """The reference's membership rule (neighborhood_search.rs:323,357,372): 1e-10 < d^2 <= h^2 with d^2 = dx dx + dy dy in fp32,
    over the fluid and the boundary particles.  -> (dynamic indices, static indices), ascending."""
    h = np.float32(h)
    out = []
    for arr in (pos, boundary):
        arr = np.asarray(arr, np.float32).reshape(-1, 2)
        d = arr - np.asarray(pos, np.float32)[i]
        d2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]
        out.append(np.nonzero((d2 <= h * h) & (d2 > np.float32(MIN_DISTANCE_SQ)))[0])
    return out
