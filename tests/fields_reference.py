"""The per-particle flow-field contract of include/sphx.h (sphx_particle_fields) restated in numpy.

* `fields32` is the contract in float32 over the downloaded neighbour lists, in the device's order of operations: entries 0 ..
  count_total - 1 in list order (dynamic, then static), every product and sum rounded once, nothing fused.  numpy evaluates every
  float32 operation correctly rounded and never fuses, so it reproduces the device bit for bit.  The lists become slot matrices
  (dfsph_reference64.Slots); column k is the k-th fp32 accumulation step of every particle.
* `fields64` forms the same sums in float64 through Restatement.pair_gradients, with their magnitudes: M_L = sum vol_j (|v_i| + |v_j|)
  g_m for every component of vel_grad, 2 M_L for divergence and vorticity (a sum / difference of two components), M_c = sum vol_j g_m
  for color_grad.  `bound_ratios` gives |f32 - f64| / (C (k + K) 2^-24 M) per output with C = 2, K = 16 — the constants
  tests/dfsph_lockstep.py uses for outputs built from a gradient times a per-neighbour factor — and k = count_total.

Inputs are the device-order arrays of an implementation: positions, velocities and densities from download(), the boundary from
download_boundary(), counts and lists from download_neighbors().  numpy only.
"""
import numpy as np

from dfsph_reference64 import Restatement, Slots, norm
from sample_reference import PI_F, powi

F = np.float32
U = 2.0 ** -24
C = 2.0
K = 16
NAMES = ("vel_grad", "divergence", "vorticity", "color_grad")


class Constants:
    """The fp32 constants of the walk, derived the way sphx_create does.  `constants6` (SphxContext.constants(): out[0] = w_hinv,
    out[2] = w_ngrad) replaces the two kernel constants by the device's own."""

    def __init__(self, params, constants6=None):
        h = F(params.smoothing_length)
        self.h = h
        self.w_hinv = F(F(1.0) / h)
        self.w_ngrad = F(F(140.0) / F(PI_F * powi(h, 4)))
        self.mass = F(params.particle_mass)
        self.rho0 = F(params.fluid_density)
        if constants6 is not None:
            c = np.asarray(constants6, F)
            self.w_hinv, self.w_ngrad = c[0], c[2]


def _arrays(state):
    pos = np.asarray(state["pos"], F).reshape(-1, 2)
    vel = np.asarray(state["vel"], F).reshape(-1, 2)
    rho = np.asarray(state["density"], F).reshape(-1)
    bnd = np.asarray(state["boundary"], F).reshape(-1, 2)
    return pos, vel, rho, bnd


def fields32(K_, state, counts, lists, boundary_neighbours=True):
    """The contract in fp32.  state: dict(pos, vel, density, boundary) in device order; counts [n, 2] and the flat lists in the
    canonical form of download_neighbors().  boundary_neighbours=False leaves the static entries out (a deliberate slip, for the
    guard of the host tests).  -> dict of the four outputs (vel_grad [n, 2, 2], color_grad [n, 2])."""
    pos, vel, rho, bnd = _arrays(state)
    n = len(pos)
    acc = {k: np.zeros(n, F) for k in ("lxx", "lxy", "lyx", "lyy", "cx", "cy")}
    if n:
        sl = Slots(np.asarray(counts).reshape(-1, 2), lists, n)
        X = np.concatenate([pos, bnd]).astype(F)
        V = np.concatenate([vel, np.zeros((len(bnd), 2), F)]).astype(F)  # v_b = (0, 0)
        with np.errstate(divide="ignore", invalid="ignore"):
            vol = np.concatenate([(K_.mass / rho).astype(F), np.full(len(bnd), F(K_.mass / K_.rho0), F)]).astype(F)
        use = sl.valid if boundary_neighbours else sl.dyn
        for k in range(use.shape[1]):
            m = use[:, k]
            if not m.any():
                continue
            j = sl.j[:, k]
            with np.errstate(invalid="ignore", over="ignore"):
                dx = (X[j, 0] - pos[:, 0]).astype(F)
                dy = (X[j, 1] - pos[:, 1]).astype(F)
                d2 = ((dx * dx).astype(F) + (dy * dy).astype(F)).astype(F)
                r = np.sqrt(d2).astype(F)
                q = np.minimum((r * K_.w_hinv).astype(F), F(1.0)).astype(F)
                omq = (F(1.0) - q).astype(F)
                s = (((K_.w_ngrad * omq).astype(F) * omq).astype(F) * omq).astype(F)
                gx, gy = (s * dx).astype(F), (s * dy).astype(F)
                ax, ay = (vol[j] * gx).astype(F), (vol[j] * gy).astype(F)
                dvx = (V[j, 0] - vel[:, 0]).astype(F)
                dvy = (V[j, 1] - vel[:, 1]).astype(F)
                for name, term in (("lxx", dvx * ax), ("lxy", dvx * ay), ("lyx", dvy * ax), ("lyy", dvy * ay)):
                    acc[name] = np.where(m, (acc[name] + term.astype(F)).astype(F), acc[name])
                acc["cx"] = np.where(m, (acc["cx"] + ax).astype(F), acc["cx"])
                acc["cy"] = np.where(m, (acc["cy"] + ay).astype(F), acc["cy"])
    grad = np.stack([acc["lxx"], acc["lxy"], acc["lyx"], acc["lyy"]], -1).astype(F).reshape(n, 2, 2)
    return dict(vel_grad=grad, divergence=(acc["lxx"] + acc["lyy"]).astype(F), vorticity=(acc["lyx"] - acc["lxy"]).astype(F),
                color_grad=np.stack([acc["cx"], acc["cy"]], -1).astype(F))


def fields64(params, state, counts, lists, particle_density=10000.0):
    """The same sums in float64 and their magnitudes.  -> (values, magnitudes, k = count_total per particle)."""
    R = Restatement.from_params(params, particle_density)
    pos, vel, rho, bnd = _arrays(state)
    n = len(pos)
    if n == 0:
        z = dict(vel_grad=np.zeros((0, 2, 2)), divergence=np.zeros(0), vorticity=np.zeros(0), color_grad=np.zeros((0, 2)))
        return z, {k: np.zeros(0) for k in NAMES}, np.zeros(0, np.int64)
    sl = Slots(np.asarray(counts).reshape(-1, 2), lists, n)
    X = np.concatenate([pos, bnd]).astype(np.float64)
    g, g_m = R.pair_gradients(X, sl)
    rho_j = np.where(sl.dyn, rho.astype(np.float64)[np.where(sl.dyn, sl.j, 0)], 1.0)
    vol = np.where(sl.dyn, R.mass / rho_j, R.mass / R.rho0) * sl.valid
    a, a_m = vol[..., None] * g, vol * g_m
    V = np.concatenate([vel, np.zeros((len(bnd), 2), F)]).astype(np.float64)
    vi, vj = V[:n], V[sl.j] * sl.dyn[..., None]
    dv = (vj - vi[:, None, :]) * sl.valid[..., None]
    L = np.einsum("isa,isb->iab", dv, a)
    M_L = ((norm(vi)[:, None] + norm(vj)) * a_m).sum(1)
    c, M_c = a.sum(1), a_m.sum(1)
    values = dict(vel_grad=L, divergence=L[:, 0, 0] + L[:, 1, 1], vorticity=L[:, 1, 0] - L[:, 0, 1], color_grad=c)
    return values, dict(vel_grad=M_L, divergence=2.0 * M_L, vorticity=2.0 * M_L, color_grad=M_c), sl.n_total


def bound_ratios(dev, ref, mag, k):
    """max over particles of |dev - ref| / (C (k + K) 2^-24 M) per output (0 where both agree exactly)."""
    out = {}
    for f in NAMES:
        if f not in dev:
            continue
        d, r = np.asarray(dev[f], np.float64), np.asarray(ref[f], np.float64)
        err = np.abs(d - r).reshape(len(d), -1).max(1) if len(d) else np.zeros(0)
        bound = C * (np.asarray(k, np.float64) + K) * U * mag[f]
        with np.errstate(invalid="ignore", divide="ignore"):
            ratio = np.where(err == 0, 0.0, err / bound)
        out[f] = float(np.max(np.where(np.isnan(ratio), np.inf, ratio))) if ratio.size else 0.0
    return out


def assert_within_bound(dev, ref, mag, k, what=""):
    r = bound_ratios(dev, ref, mag, k)
    assert all(v <= 1.0 for v in r.values()), f"{what}: float32 fields beyond the float64 round-off bound: {r}"
    return r


# ---------------------------------------------------------------------------------------------------------------- the lattice anchor
def lattice(side=32, spacing=0.01, origin=(0.5, 0.5)):
    """side x side particles at the given spacing, row-major -> (fp32 positions [side^2, 2], interior mask: particles whose whole
    support of radius h = 0.02 lies inside the lattice)."""
    ij = np.stack(np.meshgrid(np.arange(side), np.arange(side)), -1).reshape(-1, 2)
    pos = (np.asarray(origin, np.float64) + ij * float(spacing)).astype(F)
    inner = ((ij >= 3) & (ij < side - 3)).all(1)
    return pos, inner


def lattice_beta(K_, pos, density, i, counts, lists):
    """The moment factor of the discrete gradient at particle i of a lattice, in float64: beta = sum_j vol_j gx_j dx_j over i's list (by
    the lattice's symmetry the same for y, with vanishing cross moments), so that a linear field v = A x has the SPH gradient beta A."""
    pos64 = np.asarray(pos, np.float64)
    c = np.asarray(counts).reshape(-1, 2).astype(np.int64)
    start = np.concatenate([[0], np.cumsum(c[:, 1])])
    j = np.asarray(lists)[start[i]:start[i] + c[i, 0]].astype(np.int64)
    d = pos64[j] - pos64[i]
    r = np.sqrt((d * d).sum(1))
    q = np.minimum(r * float(K_.w_hinv), 1.0)
    s = float(K_.w_ngrad) * (1.0 - q) ** 3
    vol = float(K_.mass) / np.asarray(density, np.float64)[j]
    return float((vol * s * d[:, 0] * d[:, 0]).sum()), float((vol * s * d[:, 1] * d[:, 1]).sum()), float((vol * s * d[:, 0] * d[:, 1]).sum())


def host_neighbours(K_, pos, bnd=None):
    """Neighbour lists by brute force with the reference's rule (1e-10 < d2 <= h*h, d2 = dx*dx + dy*dy in fp32), ascending index,
    dynamic then static -> (counts [n, 2] uint16, flat lists uint32).  For hand-made cases of a few thousand particles."""
    pos = np.asarray(pos, F).reshape(-1, 2)
    bnd = np.zeros((0, 2), F) if bnd is None else np.asarray(bnd, F).reshape(-1, 2)
    hh = F(K_.h * K_.h)
    counts, lists = np.zeros((len(pos), 2), np.uint16), []
    for i in range(len(pos)):
        row = []
        for arr in (pos, bnd):
            d = (arr - pos[i]).astype(F)
            d2 = ((d[:, 0] * d[:, 0]).astype(F) + (d[:, 1] * d[:, 1]).astype(F)).astype(F)
            row.append(np.nonzero((d2 <= hh) & (d2 > F(1.0e-10)))[0])
        counts[i] = (len(row[0]), len(row[0]) + len(row[1]))
        lists.append(np.concatenate(row))
    return counts, (np.concatenate(lists) if lists else np.zeros(0)).astype(np.uint32)


def wendland_density(K_, pos, counts, lists, w_norm):
    """rho_i = max(rho0, m W(0) + sum_j m W(r_ij)) over the lists in float32 (FluidParticleWorld::update_densities with the Wendland kernel;
    fluid neighbours only: the anchor has no boundary)."""
    pos = np.asarray(pos, F)
    n = len(pos)
    sl = Slots(np.asarray(counts).reshape(-1, 2), lists, n)

    def w(r):
        q = np.minimum((K_.w_hinv * r).astype(F), F(1.0))
        omq = (F(1.0) - q).astype(F)
        osq = (omq * omq).astype(F)
        return (((F(w_norm) * osq).astype(F) * osq).astype(F) * (q + F(0.25)).astype(F)).astype(F)

    rho = np.full(n, F(w(np.zeros(1, F))[0] * K_.mass), F)
    for k in range(sl.valid.shape[1]):
        m = sl.valid[:, k]
        d = (pos[sl.j[:, k]] - pos).astype(F)
        r = np.sqrt(((d[:, 0] * d[:, 0]).astype(F) + (d[:, 1] * d[:, 1]).astype(F)).astype(F)).astype(F)
        rho = np.where(m, (rho + (w(r) * K_.mass).astype(F)).astype(F), rho)
    return np.maximum(rho, K_.rho0).astype(F)
