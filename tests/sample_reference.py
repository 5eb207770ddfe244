"""The field-sampling contract of include/sphx.h (sphx_sample_points / sphx_sample_grid) restated in numpy.

* `sample32` is the contract in float32, in the device's order of operations: candidates from the 3x3 cell box in ascending
  device index (fluid, then boundary), d2 = dx*dx + dy*dy unfused, accepted iff d2 <= radius_sq, sums from 0.0f in candidate order.
  numpy evaluates every float32 operation correctly rounded and never fuses, so it reproduces the device bit for bit.
* `sample64` is a float64 brute force independent of the device's grid: the particles are binned on the host in bins just above h (only
  to find everything within h of a point), accepted in float64 and summed in float64.  Every output carries a magnitude M, and
  `assert_within_bound` asserts |f32 - f64| <= C (k + K) 2^-24 M (the form of tests/dfsph_lockstep.py; k = accepted terms).
* `elevation` is the gauge rule of yasph2d_amd.gauge_elevation.

Inputs are the device-order arrays of an implementation: positions, velocities and densities from download(), the boundary from
download_boundary().  numpy only.
"""
import numpy as np

from dfsph_reference64 import Restatement

F = np.float32
PI_F = F(3.14159265358979323846)
U = 2.0 ** -24
C = 2.0
K = dict(density=8, fraction=16, velocity=16)
KERNEL_WENDLAND, KERNEL_POLY6, KERNEL_SPIKY = 0, 1, 2
FIELDS = ("density", "fraction", "velocity", "count")


def powi(a, b):
    """f32::powi as compiler-rt's __powisf2 (square-and-multiply, b > 0), as sphx_create derives the kernel constants."""
    a, r = F(a), F(1.0)
    while True:
        if b & 1:
            r = F(r * a)
        b //= 2
        if b == 0:
            return r
        a = F(a * a)


class Constants:
    """The fp32 constants of the walk, derived the way sphx_create does.  `constants6` (SphxContext.constants(): Wendland {h_inv,
    normalizer, _}, Poly6 {hsq, normalizer, _}) replaces the Wendland and Poly6 ones by the device's own."""

    def __init__(self, params, constants6=None):
        h = F(params.smoothing_length)
        self.h = h
        self.radius_sq = F(h * h)
        self.cell_inv = F(F(1.0) / h)
        self.gmin = np.array(params.grid_min[:], F)
        self.w_hinv = F(F(1.0) / h)
        self.w_norm = F(F(F(4.0) * F(7.0)) / F(PI_F * powi(h, 2)))
        self.p6_hsq = F(h * h)
        self.p6_norm = F(F(4.0) / F(PI_F * powi(h, 8)))
        self.sp_h = h
        self.sp_norm = F(F(10.0) / F(PI_F * powi(h, 5)))
        self.mass = F(params.particle_mass)
        self.rho0 = F(params.fluid_density)
        if constants6 is not None:
            c = np.asarray(constants6, F)
            self.w_hinv, self.w_norm, self.p6_hsq, self.p6_norm = c[0], c[1], c[3], c[4]


def cells_of(C_, xy):
    """cell_of: sat_u16((p - grid_min) * cell_inv) per axis (Rust `as u16`: NaN -> 0), as int64 [n, 2]."""
    with np.errstate(invalid="ignore", over="ignore"):
        v = (np.asarray(xy, F) - C_.gmin).astype(F) * C_.cell_inv
        v = np.fmin(np.fmax(v.astype(F), F(0.0)), F(65535.0))
    return v.astype(np.int64)


def _key(cx, cy):
    return (cx + 1) * 65538 + (cy + 1)


def box_pairs(q_cells, p_cells):
    """(query, particle) pairs of every particle in the 3x3 cell box of every query, sorted by (query, particle index)."""
    kp = _key(p_cells[:, 0], p_cells[:, 1])
    order = np.argsort(kp, kind="stable")
    ks = kp[order]
    qs, js = [], []
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            kq = _key(q_cells[:, 0] + dx, q_cells[:, 1] + dy)
            lo, hi = np.searchsorted(ks, kq, "left"), np.searchsorted(ks, kq, "right")
            n = hi - lo
            qi = np.repeat(np.arange(len(kq)), n)
            start = np.repeat(lo - np.concatenate(([0], np.cumsum(n)[:-1])), n)
            qs.append(qi)
            js.append(order[start + np.arange(len(qi))])
    qi, j = np.concatenate(qs), np.concatenate(js)
    o = np.lexsort((j, qi))
    return qi[o], j[o]


def w32(C_, kind, d2):
    """W(d2, r = sqrtf(d2)) in fp32, as the device evaluates it (wendland_eval / poly6_eval / spiky_eval)."""
    d2 = d2.astype(F)
    if kind == KERNEL_POLY6:
        dsq = np.maximum(F(C_.p6_hsq - d2), F(0.0)).astype(F)
        return (((C_.p6_norm * dsq).astype(F) * dsq).astype(F) * dsq).astype(F)
    r = np.sqrt(d2).astype(F)
    if kind == KERNEL_WENDLAND:
        q = np.minimum((C_.w_hinv * r).astype(F), F(1.0))
        omq = (F(1.0) - q).astype(F)
        omq_sq = (omq * omq).astype(F)
        return ((((C_.w_norm * omq_sq).astype(F) * omq_sq).astype(F)) * (q + F(0.25)).astype(F)).astype(F)
    d = np.maximum((C_.sp_h - r).astype(F), F(0.0)).astype(F)
    return (((C_.sp_norm * d).astype(F) * d).astype(F) * d).astype(F)


def _seq_sum(acc, qi, terms):
    """acc[q] = acc[q] + term, one fp32 rounding per term, in the order the terms are given (sorted by query)."""
    if len(qi) == 0:
        return acc
    first = np.concatenate(([True], qi[1:] != qi[:-1]))
    rank = np.arange(len(qi)) - np.maximum.accumulate(np.where(first, np.arange(len(qi)), 0))
    for k in range(int(rank.max()) + 1):
        sel = rank == k
        acc[qi[sel]] = (acc[qi[sel]] + terms[sel]).astype(F)
    return acc


def _accepted(C_, q, qi, pos, j):
    dx = (pos[j, 0] - q[qi, 0]).astype(F)
    dy = (pos[j, 1] - q[qi, 1]).astype(F)
    with np.errstate(invalid="ignore", over="ignore"):
        d2 = ((dx * dx).astype(F) + (dy * dy).astype(F)).astype(F)
        ok = d2 <= C_.radius_sq
    return qi[ok], j[ok], d2[ok]


def sample32(C_, state, points, kind):
    """The contract in fp32.  state: dict(pos, vel, density, boundary) in device order.  -> dict of the four outputs."""
    q = np.ascontiguousarray(points, F).reshape(-1, 2)
    m = len(q)
    pos, bnd = np.asarray(state["pos"], F), np.asarray(state["boundary"], F).reshape(-1, 2)
    qc = cells_of(C_, q)
    qi, j = box_pairs(qc, cells_of(C_, pos))
    qi, j, d2 = _accepted(C_, q, qi, pos, j)
    w = w32(C_, kind, d2)
    rho = _seq_sum(np.zeros(m, F), qi, (w * C_.mass).astype(F))
    a = ((C_.mass / np.asarray(state["density"], F)[j]).astype(F) * w).astype(F)
    frac = _seq_sum(np.zeros(m, F), qi, a)
    vel = np.asarray(state["vel"], F)
    sx = _seq_sum(np.zeros(m, F), qi, (a * vel[j, 0]).astype(F))
    sy = _seq_sum(np.zeros(m, F), qi, (a * vel[j, 1]).astype(F))
    count = np.bincount(qi, minlength=m).astype(np.uint32)
    if len(bnd):
        bqi, bj = box_pairs(qc, cells_of(C_, bnd))
        bqi, bj, bd2 = _accepted(C_, q, bqi, bnd, bj)
        rho = _seq_sum(rho, bqi, (w32(C_, kind, bd2) * C_.mass).astype(F))
    some = frac != F(0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        v = np.stack([np.where(some, (sx / frac).astype(F), F(0.0)), np.where(some, (sy / frac).astype(F), F(0.0))], -1).astype(F)
    return dict(density=rho, fraction=frac, velocity=v, count=count)


def lattice_points(x0, y0, dx, dy, nx, ny):
    """The lattice's fp32 points (x0 + (float)ix * dx, y0 + (float)iy * dy), index iy * nx + ix."""
    xs = (F(x0) + (np.arange(nx, dtype=F) * F(dx)).astype(F)).astype(F)
    ys = (F(y0) + (np.arange(ny, dtype=F) * F(dy)).astype(F)).astype(F)
    X, Y = np.meshgrid(xs, ys)
    return np.stack([X.ravel(), Y.ravel()], -1).astype(F)


# ---------------------------------------------------------------------------------------------------------------- float64 brute force
def _pairs_within(h, q, pts):
    """(query, particle) pairs with |p - q| <= h in float64: host bins just above h (no relation to the device's grid), 3x3 bins around q."""
    if len(pts) == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0)
    q64, p64 = q.astype(np.float64), pts.astype(np.float64)
    bins = h * 1.0001  # (> h: everything within h of q lies in the 3 x 3 bins around q's)
    pb = np.floor(p64 / bins)
    lo, hi = pb.min(0) - 2, pb.max(0) + 2
    with np.errstate(invalid="ignore", over="ignore"):
        qf = np.floor(q64 / bins)
        inside = (np.isfinite(qf) & (qf >= lo) & (qf <= hi)).all(1)  # (a point outside the particles' bins + 2 has nothing within h)
    qb = np.where(inside[:, None], np.where(inside[:, None], qf, 0) - lo, -10).astype(np.int64)
    pb = (pb - lo).astype(np.int64)
    qi, j = box_pairs(qb, pb)
    d = p64[j] - q64[qi]
    d2 = (d * d).sum(1)
    ok = d2 <= float(h) * float(h)
    return qi[ok], j[ok], d2[ok]


def sample64(params, state, points, kind, particle_density=10000.0):
    """The outputs in float64 (every particle within h, grid-free) and their magnitudes.  -> (values, magnitudes, terms)."""
    R = Restatement.from_params(params, particle_density)
    h = float(F(params.smoothing_length))
    mass = float(F(params.particle_mass))
    q = np.ascontiguousarray(points, F).reshape(-1, 2)
    m = len(q)
    pos, vel, rho_j = (np.asarray(state[k], np.float64) for k in ("pos", "vel", "density"))
    bnd = np.asarray(state["boundary"], F).reshape(-1, 2)
    qi, j, d2 = _pairs_within(h, q, np.asarray(state["pos"], F))
    w, wm = R.evaluate(kind, d2, np.sqrt(d2))
    rho = np.bincount(qi, w * mass, m)
    rho_m = np.bincount(qi, wm * mass, m)
    a, am = mass / rho_j[j] * w, mass / rho_j[j] * wm
    frac, frac_m = np.bincount(qi, a, m), np.bincount(qi, am, m)
    sx, sy = np.bincount(qi, a * vel[j, 0], m), np.bincount(qi, a * vel[j, 1], m)
    sv_m = np.bincount(qi, am * np.sqrt((vel[j] ** 2).sum(1)), m)
    n_fluid = np.bincount(qi, minlength=m)
    bqi, bj, bd2 = _pairs_within(h, q, bnd)
    bw, bwm = R.evaluate(kind, bd2, np.sqrt(bd2))
    rho += np.bincount(bqi, bw * mass, m)
    rho_m += np.bincount(bqi, bwm * mass, m)
    n_all = n_fluid + np.bincount(bqi, minlength=m)
    with np.errstate(invalid="ignore", divide="ignore"):
        v = np.where(frac[:, None] > 0, np.stack([sx / frac, sy / frac], -1), 0.0)
        vnorm = np.sqrt((v ** 2).sum(1))
        v_m = np.where(frac > 0, (sv_m + vnorm * frac_m) / frac, 0.0)
    return (dict(density=rho, fraction=frac, velocity=v, count=n_fluid), dict(density=rho_m, fraction=frac_m, velocity=v_m),
            dict(density=n_all, fraction=n_fluid, velocity=n_fluid))


def bound_ratios(dev, ref, mag, terms):
    """max over points of |dev - ref| / (C (k + K) 2^-24 M) per output (0 where both agree exactly)."""
    out = {}
    for f in ("density", "fraction", "velocity"):
        if f not in dev:
            continue
        d, r = np.asarray(dev[f], np.float64), np.asarray(ref[f], np.float64)
        err = np.abs(d - r)
        if err.ndim == 2:
            err = err.max(1)
        bound = C * (terms[f] + K[f]) * U * mag[f]
        with np.errstate(invalid="ignore", divide="ignore"):
            ratio = np.where(err == 0, 0.0, err / bound)
        if f == "velocity":  # (where fp32 finds no contribution the contract says (0, 0); the float64 sum may hold underflowed terms)
            ratio = np.where(np.asarray(dev["fraction"]) == 0, 0.0, ratio)
        out[f] = float(np.nanmax(np.where(np.isnan(ratio), np.inf, ratio))) if ratio.size else 0.0
    return out


def assert_within_bound(dev, ref, mag, terms, what=""):
    r = bound_ratios(dev, ref, mag, terms)
    assert all(v <= 1.0 for v in r.values()), f"{what}: float32 sampling beyond the float64 round-off bound: {r}"
    return r


# ---------------------------------------------------------------------------------------------------------------- gauge rule
def elevation(y, f):
    """The highest sample with fraction >= 0.5: its y if it is the top sample, else the float64 interpolation to 0.5 towards the
    sample above it; NaN if there is none."""
    y = np.asarray(y, np.float64)
    f = np.asarray(f, F)
    k = None
    for i in range(len(f) - 1, -1, -1):
        if f[i] >= F(0.5):
            k = i
            break
    if k is None:
        return float("nan")
    if k == len(f) - 1:
        return float(y[k])
    fk, fk1 = float(f[k]), float(f[k + 1])
    return float(y[k] + (fk - 0.5) / (fk - fk1) * (y[k + 1] - y[k]))


def gauge_column(y_lo, y_hi, dy):
    """ny = floor((y_hi - y_lo) / dy) + 1 (float64) and the fp32 sample heights y_k = fl(y_lo + fl(k * dy))."""
    ny = int(np.floor((float(y_hi) - float(y_lo)) / float(dy))) + 1
    return ny, (F(y_lo) + (np.arange(ny, dtype=F) * F(dy)).astype(F)).astype(F)
