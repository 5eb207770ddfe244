"""Lock-step comparison of a DFSPH implementation with the float64 restatement (tests/dfsph_reference64.py).

An implementation (the oracle's or the device's tile backend, one tile over the whole domain) runs a plan of sub-steps in the call
order of tiles_reference.TiledDFSPH.step; its state is downloaded after every sub-step (`run_plan` -> trace).  `check_trace` then
applies the restatement to the state BEFORE each sub-step and compares what it predicts with the state AFTER it, particle by
particle, within

    |dev - ref| <= C (n + K) 2^-24 M

n = the particle's neighbour count, K = a small per-operation allowance (the roundings outside the neighbour sum), M = the
restatement's magnitude of that output (the same expression in absolute values, cancelling subtractions at operand size), C = one
constant.  Replaying a recorded trace through a mutated restatement must FAIL the same comparison (tests of the sensitivity)."""
import numpy as np

from dfsph_reference64 import Restatement, brute_force_neighbors

U = 2.0 ** -24
C = 2.0
# roundings outside the neighbour sum, per output
K = dict(density=8, alpha=16, vmax_sq=16, predict=12, k=16, velocity=16, residual=8, position=4,
         # WCSPH (tests/wcsph_lockstep.py), counted on the Rust expressions as the entries above were:
         # wscsph.rs:93-105 per neighbour: ri_to_rj 1, r_sq 3, sqrt 1, pi + pj 1, -mass * 1, 2 rhoi rhoj 2, / 1, h - r 1, n_grad hsubr hsubr 2,
         # r + eps 1, / 1, * ri_to_rj 1, pressure_unsmoothed * 1, += 1 (18); the viscous term (xsph.rs:22 with poly6.rs:24-28, the
         # longer of the two models): hsq - r_sq 1, n d d d 3, eps * m 1, * W 1, rhoj * dt 1, / 1, vj - vi 1, * 1, += 1 (11); the two
         # pressures' own roundings are in their magnitude.  29 -> 32.
         wcsph_accel=32,
         # wscsph.rs:148-149 from the state before: 0.5 dt exact, * a 1, v += 1, v * dt 1, pos += 1.  4.
         leapfrog=4,
         # wscsph.rs:162 from an implementation's own v and a: a * dt 1, v + 1, magnitude2 3 (5), each of the first two doubled in the
         # square (7).  -> 8.
         wcsph_vmax_sq=8,
         # wscsph.rs:176 on the restated accelerations: 0.5 * dt 0, * a 1, += 1 on top of the accelerations' own 32.  -> 36.
         wcsph_velocity=36)
WHOLE_DOMAIN = (0, 65536, 0, 65536)
PARTICLE_DENSITY = 10000.0  # the default_params() argument the parameter block was made with


def restatement(params=None, particle_density=PARTICLE_DENSITY):
    """The restatement for a parameter block and the particle density it was made with (default: the reference app's)."""
    import yasph2d_amd as y

    return Restatement.from_params(y.default_params() if params is None else params, particle_density)


class Bounds:
    """Collects |dev - ref| / bound per output; remembers the worst particle of each."""

    def __init__(self):
        self.worst = {}

    def check(self, name, dev, ref, m, n, k, ids=None, where=""):
        dev, ref, m = np.asarray(dev, np.float64), np.asarray(ref, np.float64), np.asarray(m, np.float64)
        err = np.abs(dev - ref)
        if err.ndim == 2:
            err = err.max(1)
        if err.size == 0:
            return 0.0
        bound = C * (np.asarray(n, np.float64) + K[k]) * U * m
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(err == 0, 0.0, err / bound)
        ratio = np.where(np.isnan(dev).any(-1) if dev.ndim == 2 else np.isnan(dev), np.inf, ratio)
        i = int(np.argmax(ratio))
        r = float(ratio[i])
        if r > self.worst.get(name, (-1.0,))[0]:
            nn = np.broadcast_to(np.asarray(n), ratio.shape)[i]
            self.worst[name] = (r, dict(where=where, particle=i, id=None if ids is None else int(ids[i]), neighbors=int(nn),
                                        dev=dev[i].tolist(), ref=ref[i].tolist(), bound=float(np.broadcast_to(bound, ratio.shape)[i])))
        return r

    def max_ratio(self):
        return max((v[0] for v in self.worst.values()), default=0.0)

    def report(self):
        return "\n".join(f"  {k}: ratio {v[0]:.3g} at {v[1]}" for k, v in sorted(self.worst.items(), key=lambda kv: -kv[1][0]))

    def assert_within(self):
        assert self.max_ratio() <= 1.0, "restatement and implementation disagree beyond the round-off bound:\n" + self.report()


# ---------------------------------------------------------------------------------------------------------------------- running
def lists_of(backend):
    if hasattr(backend, "o"):
        return backend.o.neighbors()
    return backend.ctx.download_neighbors()


def boundary_of(backend):
    """The implementation's (sorted) boundary array: static list entries index it."""
    if hasattr(backend, "o"):
        return backend.o.boundary()
    return backend.ctx.download_boundary()[0]


def snapshot(backend, boundary, lists=None):
    d = backend.download()
    s = {k: np.array(d[k], copy=True) for k in ("pos", "vel", "density", "alpha", "kappa", "stiffness", "ids")}
    s["boundary"] = boundary_of(backend) if boundary is None else boundary
    if lists is False:  # before the first re-grid: no lists yet
        lists = (np.zeros((len(s["pos"]), 2), np.uint16), None, np.zeros(0, np.uint32))
    s["counts"], _, s["lists"] = lists if lists is not None else lists_of(backend)
    return s


def single_tile(backend, pos, vel, boundary, kappa=None, stiffness=None):
    """One tile that covers the whole domain, no peers: every particle owned, no ghosts."""
    boundary = np.ascontiguousarray(boundary, np.float32).reshape(-1, 2)
    if len(boundary):
        backend.set_boundary(boundary)
    backend.configure(WHOLE_DOMAIN, 16, [])
    backend.reserve(len(pos) + 4096)
    ids = np.arange(len(pos), dtype=np.uint32)
    if kappa is not None:  # oracle only: a state with live warm-start values
        backend._set(pos, vel, ids | np.uint32(0x80000000), kappa, stiffness)
    else:
        backend.upload(pos, np.zeros_like(pos) if vel is None else vel, ids)
    return boundary


def make_plan(steps, fixed=(3, 2), dts=((0.003, 0.002), (0.002, 0.0025), (0.0025, 0.0015)), warm_from=1, fuse_predict=False, regrid="plain",
              dt_scale=1.0):
    """Sub-steps of `steps` DFSPH steps (TiledDFSPH.step order).  Warm starts fire from step `warm_from` on (both loops).  regrid:
    "plain" (sphx_sub_regrid), or the device's fused forms "fused" (_div before a cold divergence loop, _warm before a warm one).
    dt_scale: factor on `dts` (particle spacing / 0.01 for a parameter set of another resolution)."""
    nd, nv = fixed
    plan = [("regrid",)]
    for s in range(steps):
        dt_prev, dt = (np.float32(x) * np.float32(dt_scale) for x in dts[s % len(dts)])
        warm = s >= warm_from
        plan.append(("nonpressure", dt_prev))
        if fuse_predict and not warm:
            plan.append(("predict_iteration", dt, dt_prev))
            first = 1
        else:
            plan.append(("predict", dt, dt_prev))
            if warm:
                plan.append(("warmstart", 0, dt))
            first = 0
        plan += [("iteration", 0, dt, i == 0) for i in range(first, nd)]
        plan.append(("advect", dt))
        if regrid == "fused":
            plan.append(("regrid_warm", dt) if warm else ("regrid_div",))
            if warm:
                plan.append(("warmstart_noop", 1, dt))
        else:
            plan.append(("regrid",))
            if warm:
                plan.append(("warmstart", 1, dt))
        plan += [("iteration", 1, dt, i == 0) for i in range(nv)]
    return plan


def _call(backend, op):
    import ctypes as Cx

    name = op[0]
    if name == "regrid":
        return backend.regrid()
    if name in ("regrid_div", "regrid_warm"):
        n = Cx.c_uint32()
        fn = backend.L.sphx_sub_regrid_div if name == "regrid_div" else backend.L.sphx_sub_regrid_warm
        backend._chk(fn(backend.ctx.h, Cx.byref(n)))
        return n.value
    if name == "nonpressure":
        return backend.nonpressure(op[1])
    if name == "predict":
        return backend.predict(op[1])
    if name == "predict_iteration":
        s, n = Cx.c_double(), Cx.c_uint64()
        backend._chk(backend.L.sphx_sub_predict_iteration(backend.ctx.h, op[1], Cx.byref(s), Cx.byref(n)))
        return s.value, n.value
    if name in ("warmstart", "warmstart_noop"):
        return backend.warmstart(op[1], op[2])
    if name == "iteration":
        return backend.iteration(op[1], op[2], op[3])
    if name == "advect":
        return backend.advect(op[1])
    raise ValueError(name)


def run_plan(backend, plan, record=True):
    """Runs the plan; with record, downloads the state after every sub-step.  -> trace [(op, returned, before, after)] (record) or
    the final snapshot."""
    trace = []
    pre = snapshot(backend, None, False if plan[0][0].startswith("regrid") else None) if record else None
    for op in plan:
        ret = _call(backend, op)
        if record:
            fresh = op[0].startswith("regrid")
            post = snapshot(backend, None if fresh else pre["boundary"], None if fresh else (pre["counts"], None, pre["lists"]))
            trace.append((op, ret, pre, post))
            pre = post
    backend.synchronize()
    return trace if record else snapshot(backend, None)


def run_and_check(backend, plan, ref, bounds, where="", rows=None):
    """run_plan + check_trace one sub-step at a time, keeping two snapshots (for contexts too large to record a whole trace)."""
    pre = snapshot(backend, None, False if plan[0][0].startswith("regrid") else None)
    for i, op in enumerate(plan):
        ret = _call(backend, op)
        fresh = op[0].startswith("regrid")
        post = snapshot(backend, None if fresh else pre["boundary"], None if fresh else (pre["counts"], None, pre["lists"]))
        check_trace([(op, ret, pre, post)], ref, bounds, f"{where} #{i}", rows)
        pre = post
    return pre


# --------------------------------------------------------------------------------------------------------------------- checking
def _by_id(post_ids, pre_ids):
    inv = np.full(int(max(pre_ids.max(initial=0), post_ids.max(initial=0))) + 1, -1, np.int64)
    inv[pre_ids] = np.arange(len(pre_ids))
    perm = inv[post_ids]
    assert (perm >= 0).all(), "a re-grid lost or invented a particle"
    return perm


def _combined(s):
    return np.concatenate([s["pos"], np.asarray(s["boundary"], np.float32).reshape(-1, 2)]).astype(np.float64)


def _abs(x):
    return np.abs(np.asarray(x, np.float64))


def check_trace(trace, ref, bounds, where="", rows=None, model=None):
    """Applies `ref` to every recorded sub-step; the ratios go to `bounds`.  rows: compare these particles (slots) only — the
    residual sums and vmax, which need every particle, are then not compared.  model: ("xsph", epsilon) or ("physical", mu), handed
    to ref.nonpressure (None: the model `ref` was made with)."""
    acc, folded = None, False
    for step, (op, ret, pre, post) in enumerate(trace):
        name = op[0]
        tag = f"{where} #{step} {name}"
        n_fluid = len(pre["pos"])
        X = _combined(pre)
        r = slice(None) if rows is None else rows
        ids = pre["ids"][r]
        if not name.startswith("regrid"):
            sl = ref.slots(pre["counts"], pre["lists"], n_fluid, rows)
            n = sl.n_total
        if name.startswith("regrid"):
            Xa = _combined(post)
            sla = ref.slots(post["counts"], post["lists"], len(post["pos"]), rows)
            rho, rho_m = ref.update_densities(Xa, sla)
            bounds.check("density", post["density"][r], rho, rho_m, sla.n_total, "density", post["ids"][r], tag)
            alpha, alpha_m = ref.compute_alpha_factors(Xa, sla)
            bounds.check("alpha", post["alpha"][r], alpha, alpha_m, sla.n_total, "alpha", post["ids"][r], tag)
            perm = _by_id(post["ids"], pre["ids"])
            assert np.array_equal(post["pos"].view(np.uint32), pre["pos"][perm].view(np.uint32)), tag + ": a re-grid moved particles"
            unchanged = np.array_equal(post["vel"].view(np.uint32), pre["vel"][perm].view(np.uint32))
            if name == "regrid_warm":  # the build applied the divergence warm start (dfsph.rs:354-360) to the re-sorted particles ...
                folded = not unchanged   # ... unless SPHX_FUSE_WARM=0: then the sphx_sub_warmstart call that follows does
                if folded:
                    v, v_m, _ = ref.warm_start(Xa, pre["vel"][perm], pre["stiffness"][perm], sla, float(op[1]), True)
                    bounds.check("velocity", post["vel"][r], v, v_m, sla.n_total, "velocity", post["ids"][r], tag)
            else:
                assert unchanged, tag + ": a re-grid changed velocities"
        elif name == "nonpressure":
            dt_prev = float(op[1])
            acc = ref.nonpressure(X, pre["vel"], pre["density"], sl, dt_prev, model)
            if rows is None:
                vsq, vsq_m = ref.max_velocity_sq(pre["vel"], acc[0], acc[1], dt_prev)
                bounds.check("vmax_sq", [ret], [vsq], [vsq_m], [n.max(initial=0)], "vmax_sq", None, tag)
            assert np.array_equal(post["vel"].view(np.uint32), pre["vel"].view(np.uint32)), tag + ": the non-pressure pass changed v"
        elif name in ("predict", "predict_iteration"):
            dt = float(op[1])
            # (the state of the non-pressure pass, unchanged)
            acc = ref.nonpressure(X, pre["vel"], pre["density"], sl, float(op[2]), model)
            vs, vs_m = ref.predict(pre["vel"][r], acc[0], acc[1], dt)
            if name == "predict":
                bounds.check("predict", post["vel"][r], vs, vs_m, n, "predict", ids, tag)
            else:
                assert rows is None, "the fused prediction needs v* of the neighbours"  # + the first density iteration from zeroed warm starts, on the float64 prediction
                k, k_m, e, e_m = ref.density_iteration_k(X, vs, pre["density"], pre["alpha"], sl, dt)
                kd = post["kappa"]
                bounds.check("k_density", kd, k, k_m + _abs(kd), n, "k", ids, tag)
                v, v_m = ref.correct_velocity(X, vs, kd, _abs(kd), sl, 1.0 / dt)
                bounds.check("velocity", post["vel"], v, v_m + vs_m, n, "velocity", ids, tag)
                bounds.check("residual_sum", [ret[0]], [e.sum()], [e_m.sum()], [n.max(initial=0) + np.log2(max(2, n_fluid))], "residual", None, tag)
        elif name == "warmstart" or (name == "warmstart_noop" and not folded):
            div, dt = int(op[1]), float(op[2])
            key = "stiffness" if div else "kappa"
            # (what the array holds afterwards is not compared: the loop zeroes it before anything reads it, dfsph.rs:206 / :361)
            v, v_m, _ = ref.warm_start(X, pre["vel"], pre[key], sl, dt, bool(div))
            bounds.check("velocity", post["vel"][r], v, v_m, n, "velocity", ids, tag)
        elif name == "warmstart_noop":
            assert np.array_equal(post["vel"].view(np.uint32), pre["vel"].view(np.uint32)), tag + ": the folded warm start ran twice"
        elif name == "iteration":
            div, dt, first = int(op[1]), float(op[2]), bool(op[3])
            key = "stiffness" if div else "kappa"
            kb = np.zeros(n_fluid) if first else pre[key].astype(np.float64)
            ka = post[key].astype(np.float64)
            kdev = ka - kb
            if div:
                k, k_m, e, e_m = ref.divergence_iteration_k(X, pre["vel"], pre["alpha"], sl)
            else:
                k, k_m, e, e_m = ref.density_iteration_k(X, pre["vel"], pre["density"], pre["alpha"], sl, dt)
            kmag = _abs(ka) + _abs(kb)  # kappa_after = fl(kappa_before + k)
            bounds.check("k_divergence" if div else "k_density", kdev[r], k, k_m + kmag[r], n, "k", ids, tag)
            v, v_m = ref.correct_velocity(X, pre["vel"], kdev, kmag, sl, 1.0 if div else 1.0 / dt)
            bounds.check("velocity", post["vel"][r], v, v_m, n, "velocity", ids, tag)
            if rows is None:
                bounds.check("residual_sum", [ret[0]], [e.sum()], [e_m.sum()], [n.max(initial=0) + np.log2(max(2, n_fluid))], "residual",
                             None, tag)
            assert np.array_equal(post["pos"].view(np.uint32), pre["pos"].view(np.uint32)), tag + ": an iteration moved particles"
        elif name == "advect":
            x, x_m = ref.advect(pre["pos"][r], pre["vel"][r], float(op[1]))
            bounds.check("position", post["pos"][r], x, x_m, 0, "position", ids, tag)
        else:
            raise ValueError(name)
    return bounds


def check_membership(s, h, sample=64, seed=0, grid_min=(-100.0, -100.0)):
    """For a seeded sample of particles: an uncapped list is exactly the brute-force set of the reference rule, dynamic entries
    ascending then static entries ascending; a capped list (64 entries) holds members of it only."""
    counts, lists = s["counts"], s["lists"]
    start = np.zeros(len(counts) + 1, np.int64)
    np.cumsum(counts[:, 1].astype(np.int64), out=start[1:])
    n = len(counts)
    rng = np.random.default_rng(seed)
    # not in the domain's rim cells, where the reference's neighbour box wraps (neighborhood_search.rs:193-194: pos.x - 1 at x = 0)
    gm = np.asarray(grid_min, np.float64)
    lo, hi = (gm + 2 * h).astype(np.float32), (gm + 65534 * h).astype(np.float32)
    inner = np.nonzero(((s["pos"] > lo) & (s["pos"] < hi)).all(1))[0]
    picks = rng.choice(inner, min(sample, len(inner)), replace=False) if len(inner) else []
    for i in picks:
        nd, nt = int(counts[i, 0]), int(counts[i, 1])
        entries = lists[start[i]:start[i + 1]].astype(np.int64)
        dyn, stat = brute_force_neighbors(s["pos"], s["boundary"], h, i)
        if nt < 64:
            assert np.array_equal(entries[:nd], dyn) and np.array_equal(entries[nd:], stat), (
                f"particle {i}: list {entries.tolist()} (dynamic {nd}) vs brute force {dyn.tolist()} + {stat.tolist()}")
        else:
            assert np.isin(entries[:nd], dyn).all() and np.isin(entries[nd:], stat).all(), f"particle {i}: capped list has non-members"


def membership_of_trace(trace, h, seed=0, grid_min=(-100.0, -100.0)):
    for op, _, _, post in trace:
        if op[0].startswith("regrid"):
            check_membership(post, h, seed=seed, grid_min=grid_min)


# ---------------------------------------------------------------------------------------------------------------------- mutants
class DropLastEntry(Restatement):
    """the last entry of every neighbour list dropped"""

    def slots(self, counts, lists, n_fluid, rows=None):
        from dfsph_reference64 import Slots

        return Slots(counts, lists, n_fluid, rows, drop=1)


class BoundaryScaled(Restatement):
    """every boundary (static) term scaled by 1.001"""

    def _scale(self, sl):
        return np.where(sl.stat, 1.001, 1.0)

    def pair_gradients(self, X, sl):
        g, m = super().pair_gradients(X, sl)
        return g * self._scale(sl)[..., None], m * self._scale(sl)

    def pair_kernel(self, X, sl, kind):
        w, m = super().pair_kernel(X, sl, kind)
        return w * self._scale(sl), m * self._scale(sl)


class AlphaWithoutMass(Restatement):
    """alpha from grad W instead of m grad W"""

    def compute_alpha_factors(self, X, sl):
        mass, self.mass = self.mass, 1.0
        try:
            return super().compute_alpha_factors(X, sl)
        finally:
            self.mass = mass


class DensityErrorWithDtPrev(Restatement):
    """dt_prev in place of dt in compute_density_error"""

    def nonpressure(self, X, V, rho, sl, dt_prev, model=None):
        self.dt_prev = dt_prev
        return super().nonpressure(X, V, rho, sl, dt_prev, model)

    def compute_density_error(self, X, V, rho, sl, dt):
        return super().compute_density_error(X, V, rho, sl, self.dt_prev)


class GateAtMostNine(Restatement):
    """the particle-deficiency gate as <= 9"""

    def deficient(self, n_total):
        return n_total <= 9


class DivergenceOnPreAdvectPositions(Restatement):
    """the divergence walk on the positions before the advection"""

    def predict(self, V, acc, acc_m, dt):
        self.dt = dt
        return super().predict(V, acc, acc_m, dt)

    def compute_density_change(self, X, V, sl):
        X = np.array(X, np.float64)
        X[:len(V)] -= np.asarray(V, np.float64) * self.dt
        return super().compute_density_change(X, V, sl)


class GradientNormH3(Restatement):
    """the Wendland gradient normaliser derived with h^3 instead of h^4"""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.wendland_grad_norm = 140.0 / (np.pi * self.h ** 3)


class GradientSquare(Restatement):
    """the Wendland gradient's (1 - q)^3 as (1 - q)^2"""

    def grad_shape(self, q):
        from dfsph_reference64 import power_of_difference

        return power_of_difference(1.0 - q, q, 2)


class NoWarmStartDamping(Restatement):
    """the warm start without its 0.5 max(k, -0.5 rho0^2) damping"""

    def damp(self, k):
        return np.asarray(k, np.float64)


MUTANTS = [DropLastEntry, BoundaryScaled, AlphaWithoutMass, DensityErrorWithDtPrev, GateAtMostNine, DivergenceOnPreAdvectPositions,
           GradientNormH3, GradientSquare, NoWarmStartDamping]


def mutant(cls, params=None, particle_density=PARTICLE_DENSITY):
    import yasph2d_amd as y

    return cls.from_params(y.default_params() if params is None else params, particle_density)


# ------------------------------------------------------------------------------------------------------------------ whole steps
def context_state(ctx):
    """pos, vel, density, alpha, kappa, stiffness, ids, lists and boundary of a SphxContext (or an Oracle)."""
    if hasattr(ctx, "dfsph_step"):  # oracle
        s = dict(pos=ctx.positions(), vel=ctx.velocities(), density=ctx.densities(), ids=ctx.ids(), alpha=ctx.alpha(),
                 kappa=ctx.kappa(), stiffness=ctx.stiffness(), boundary=ctx.boundary())
        s["counts"], _, s["lists"] = ctx.neighbors()
        return s
    d = ctx.download()
    s = dict(pos=d["pos"], vel=d["vel"], density=d["density"], ids=d["ids"], boundary=ctx.download_boundary()[0])
    s.update(ctx.download_solver_state())
    s["counts"], _, s["lists"] = ctx.download_neighbors()
    return s


def restate_step(ref, pre, post, dt_prev, dt, iterations, warm):
    """One whole simulation_step (dfsph.rs:414-525) in float64 from the state before it.  The re-sort is the implementation's: the
    second half runs in its post-step order (ids) on its post-step lists.  Warm-start values stay in their slots over the re-sort
    (dfsph.rs:512: only positions and velocities travel).  -> dict of the outputs."""
    nd, nv = iterations
    n = len(pre["pos"])
    X = _combined(pre)
    sl = ref.slots(pre["counts"], pre["lists"], n)
    acc, acc_m = ref.nonpressure(X, pre["vel"], pre["density"], sl, dt_prev)
    vmax_sq, _ = ref.max_velocity_sq(pre["vel"], acc, acc_m, dt_prev)
    v, _ = ref.predict(pre["vel"], acc, acc_m, dt)
    if warm[0]:
        v = ref.warm_start(X, v, pre["kappa"], sl, dt, False)[0]
    kappa, avgs_d = np.zeros(n), []
    for _ in range(nd):
        k, _, e, _ = ref.density_iteration_k(X, v, pre["density"], pre["alpha"], sl, dt)
        kappa += k
        v = ref.correct_velocity(X, v, k, np.abs(k), sl, 1.0 / dt)[0]
        avgs_d.append(ref.average_density_error(e))
    x, _ = ref.advect(pre["pos"], v, dt)
    perm = _by_id(post["ids"], pre["ids"])
    x, v = x[perm], v[perm]
    Xn = np.concatenate([x, np.asarray(post["boundary"], np.float64).reshape(-1, 2)])
    sln = ref.slots(post["counts"], post["lists"], n)
    rho, _ = ref.update_densities(Xn, sln)
    alpha, _ = ref.compute_alpha_factors(Xn, sln)
    if warm[1]:
        v = ref.warm_start(Xn, v, pre["stiffness"], sln, dt, True)[0]
    stiff, avgs_v = np.zeros(n), []
    for _ in range(nv):
        k, _, c, _ = ref.divergence_iteration_k(Xn, v, alpha, sln)
        stiff += k
        v = ref.correct_velocity(Xn, v, k, np.abs(k), sln, 1.0)[0]
        avgs_v.append(ref.average_divergence(c))
    return dict(pos=x, vel=v, density=rho, alpha=alpha, kappa=kappa, stiffness=stiff, vmax_sq=vmax_sq, avg_density_error=avgs_d[-1],
                avg_divergence=avgs_v[-1], avgs_density=avgs_d, avgs_divergence=avgs_v)


STEP_FIELDS = ("pos", "vel", "density", "alpha", "kappa", "stiffness")


def step_deviation(out, post, stats):
    """Relative deviation per output: max |dev - ref| / max |ref| (positions: relative to the step's largest displacement)."""
    dev = {}
    for k in STEP_FIELDS:
        a, b = np.asarray(post[k], np.float64), out[k]
        if k == "pos":
            dev[k] = float(np.abs(a - b).max() / max(np.abs(out["vel"]).max() * stats["dt"], 1e-30))
        else:
            dev[k] = float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))
    dev["vmax"] = abs(stats["vmax"] ** 2 - out["vmax_sq"]) / out["vmax_sq"]
    dev["avg_density_error"] = abs(stats["avg_density_error"] - out["avg_density_error"]) / max(abs(out["avg_density_error"]), 1e-30)
    dev["avg_divergence"] = abs(stats["avg_divergence"] - out["avg_divergence"]) / max(abs(out["avg_divergence"]), 1e-30)
    return dev
