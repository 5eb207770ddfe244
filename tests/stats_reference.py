"""numpy restatement of sphx_fluid_stats (include/sphx.h, "fluid statistics"): the terms formed in float64 from the float32 values exactly
as the header writes them, exact sums by math.fsum, exact counts and extremes, the rectangle predicate in float32.

stats(d, rects, density_valid) -> one dict per record (record 0 = everything, record 1 + k = rects[k]) with the members of sphx_stats_rec
plus, per sum, "abs_<name>" = fsum(|t|) and the number of terms — what the stated error bound n * 2^-52 * sum|t| is made of.
check(got, want) compares one device record with one reference record by the contract: counts, extremes and max_speed_sq bit for bit,
every sum within the stated bound of the exact sum."""
import math

import numpy as np

F = np.float32
SUMS = ("sum_pos", "sum_vel", "sum_speed_sq", "sum_angular", "sum_density", "sum_density_sq")  # members that are float64 sums
EXACT = ("count", "nonfinite", "density_count", "density_valid", "reserved", "max_speed_sq", "min_pos", "max_pos", "min_density", "max_density")
U = 2.0 ** -52


def inside(pos, r):
    """in(r, p) = p.x >= r.x0 && p.x < r.x1 && p.y >= r.y0 && p.y < r.y1 in float32 — a NaN coordinate fails every comparison"""
    x0, y0, x1, y1 = (F(v) for v in r)
    with np.errstate(invalid="ignore"):
        return (pos[:, 0] >= x0) & (pos[:, 0] < x1) & (pos[:, 1] >= y0) & (pos[:, 1] < y1)


def _min(a):
    """the exact minimum of finite float32 values, -0 below +0; +inf for none"""
    if len(a) == 0:
        return F(np.inf)
    m = a.min()
    return F(-0.0) if m == 0 and np.signbit(a[a == 0]).any() else F(m)


def _max(a):
    if len(a) == 0:
        return F(-np.inf)
    m = a.max()
    return F(0.0) if m == 0 and (~np.signbit(a[a == 0])).any() else F(m)


def _fsum(t):
    return math.fsum(t.tolist()), math.fsum(np.abs(t).tolist()), len(t)


def record(pos, vel, density, member, density_valid):
    pos, vel = np.asarray(pos, F).reshape(-1, 2), np.asarray(vel, F).reshape(-1, 2)
    member = np.asarray(member, bool)
    fin = np.isfinite(pos).all(axis=1) & np.isfinite(vel).all(axis=1)
    sel = member & fin
    x, yy, vx, vy = (a[sel].astype(np.float64) for a in (pos[:, 0], pos[:, 1], vel[:, 0], vel[:, 1]))
    speed = vx * vx + vy * vy  # (each product is exact in float64: one rounding per term, fused or not)
    ang = x * vy - yy * vx
    r = dict(count=int(sel.sum()), nonfinite=int((member & ~fin).sum()), density_valid=int(bool(density_valid)), reserved=0)
    sums = dict(sum_pos=(x, yy), sum_vel=(vx, vy), sum_speed_sq=(speed,), sum_angular=(ang,))
    if density_valid:
        dsel = sel & np.isfinite(np.asarray(density, F))
        rho32 = np.asarray(density, F)[dsel]
        rho = rho32.astype(np.float64)
    else:
        rho32, rho = np.zeros(0, F), np.zeros(0)
    r["density_count"] = len(rho)
    sums.update(sum_density=(rho,), sum_density_sq=(rho * rho,))
    for name, terms in sums.items():
        got = [_fsum(t) for t in terms]
        r[name] = np.array([g[0] for g in got]) if len(got) > 1 else got[0][0]
        r["abs_" + name] = np.array([g[1] for g in got]) if len(got) > 1 else got[0][1]
        r["n_" + name] = got[0][2]
    r["max_speed_sq"] = float(speed.max()) if len(speed) else 0.0
    r["min_pos"] = np.array([_min(pos[sel, 0]), _min(pos[sel, 1])], F)
    r["max_pos"] = np.array([_max(pos[sel, 0]), _max(pos[sel, 1])], F)
    r["min_density"], r["max_density"] = _min(rho32), _max(rho32)
    return r


def stats(d, rects=(), density_valid=True):
    """d: a ctx.download() dict (pos, vel, density) or (pos, vel, density); rects: (x0, y0, x1, y1) tuples"""
    pos, vel, density = (d["pos"], d["vel"], d["density"]) if isinstance(d, dict) else d
    pos = np.asarray(pos, F).reshape(-1, 2)
    rects = np.asarray(rects, F).reshape(-1, 4)
    out = [record(pos, vel, density, np.ones(len(pos), bool), density_valid)]
    for r in rects:
        out.append(record(pos, vel, density, inside(pos, r), density_valid))
    return out


def bits(v):
    a = np.atleast_1d(np.asarray(v))
    return a.view(np.uint64 if a.dtype.itemsize == 8 else np.uint32).tolist()


def check(got, want, what="", slack=1.0):
    """got: one element of the device's structured array; want: one reference record.  slack multiplies the stated bound (2 where the
    contract compares two device sums with each other)."""
    for k in EXACT:
        g = np.asarray(got[k])
        w = np.asarray(want[k], g.dtype)
        assert bits(g) == bits(w), "%s: %s is %r, expected %r" % (what, k, g.tolist(), w.tolist())
    for k in SUMS:
        g, w, a = np.atleast_1d(got[k]), np.atleast_1d(want[k]), np.atleast_1d(want["abs_" + k])
        for j in range(len(g)):
            bound = slack * want["n_" + k] * U * a[j]
            assert abs(float(g[j]) - float(w[j])) <= bound, "%s: %s[%d] is %r, exact %r: off by %.3g, bound %.3g" % (
                what, k, j, float(g[j]), float(w[j]), abs(float(g[j]) - float(w[j])), bound)
