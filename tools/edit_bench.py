#!/usr/bin/env python3
"""Cost of editing the particle set on the device (sphx_remove / sphx_append) next to the round trip they replace.

  tools/edit_bench.py [--particles 1000000] [--warmup 50] [--calls 9] [--out profiles/edit/edit_<n>.json]

The dam-break scene is stepped --warmup times; on that state, --calls times each (the state is put back by a fresh upload of the same
arrays in between, so every call sees the same particles):
  * sphx_remove with 0 %, 1 % and 50 % removed (a half plane x >= the matching quantile of the positions);
  * sphx_append of 4096 particles into reserved room (in place) and into exact capacity (the arrays grow by half);
  * the round trip: download + numpy filter (1 % removed) + upload.
Per case: the median wall time of the call (us; it includes the call's one synchronisation), the device time of its launches by label
(sphx_profile_*, median per call), and for sphx_remove the achieved bandwidth against the byte model 8 B per particle read for the
predicate + 40 B per survivor moved (nothing is moved when nothing goes).  Prints one JSON line and writes it to --out."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import yasph2d_amd as y  # noqa: E402

INF = float("inf")
LABELS = ("remove_flag", "remove_scan", "remove_move", "append")


def fresh(pos, vel, boundary, reserve=0):
    ctx = y.SphxContext()
    if reserve:
        ctx._chk(ctx.L.sphx_reserve(ctx.h, reserve))
    ctx.set_boundary(boundary)
    ctx.upload(pos, vel)
    return ctx


def timed(ctx, calls, restore, fn):
    """median wall time of fn (us) and the median device time per label (us)"""
    wall, dev = [], {k: [] for k in LABELS}
    for _ in range(calls):
        restore()
        ctx.synchronize()
        ctx.profile_reset()
        t0 = time.perf_counter()
        fn()
        wall.append((time.perf_counter() - t0) * 1e6)
        ctx.synchronize()
        prof = ctx.profile_get()
        for k in LABELS:
            if k in prof:
                dev[k].append(prof[k]["total_ms"] * 1e3)
    return float(np.median(wall)), {k: float(np.median(v)) for k, v in dev.items() if v}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", type=int, default=1_000_000)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--calls", type=int, default=9)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    w = y.FluidParticleWorld()
    w.reset_fluid(float(np.sqrt(args.particles / 4050.0)))
    boundary = w.boundary_particles
    s = y.DFSPHSolver(w, y.default_params())
    s.simulation_steps(w, y.TimeManager(), args.warmup, sync_world=False)
    d = s.context().download(density=False, ids=False)
    s.close()
    pos, vel = d["pos"], d["vel"]
    n = len(pos)
    out = dict(particles=n, warmup=args.warmup, calls=args.calls)
    ctx = fresh(pos, vel, boundary)
    ctx.profile_filter(None)
    ctx.profile_enable(True)
    out["event_overhead_us"] = ctx.profile_event_overhead() * 1e3
    xs = np.sort(pos[:, 0])
    for name, frac in (("remove_0pct", 0.0), ("remove_1pct", 0.01), ("remove_50pct", 0.5)):
        x0 = INF if frac == 0.0 else float(xs[n - int(round(frac * n))])
        removed = []
        wall, dev = timed(ctx, args.calls, lambda: ctx.upload(pos, vel), lambda: removed.append(ctx.remove((x0, -INF, INF, INF))))
        kept = n - removed[-1]
        device_us = sum(dev.values())
        model = 8.0 * n + (40.0 * kept if removed[-1] else 0.0)
        out[name] = dict(removed=removed[-1], wall_us=wall, device_us=device_us, by_label_us=dev, model_bytes=model,
                         achieved_TB_per_s=model / (device_us * 1e-6) / 1e12)
    # the round trip the calls replace, removing the same 1 %
    x1 = float(xs[n - int(round(0.01 * n))])

    def round_trip():
        t = ctx.download(density=False, ids=False)
        keep = ~(t["pos"][:, 0] >= np.float32(x1))
        ctx.upload(t["pos"][keep], t["vel"][keep])

    wall, _ = timed(ctx, max(3, args.calls // 3), lambda: ctx.upload(pos, vel), round_trip)
    out["round_trip_1pct"] = dict(wall_us=wall)
    out["round_trip_over_remove_1pct"] = wall / out["remove_1pct"]["wall_us"]
    ctx.close()
    # sphx_append of 4096 particles: in place (reserved room) and with growth (exact capacity; a fresh context per call)
    extra = (pos[:4096] + np.float32(0.001)).astype(np.float32)
    ctx = fresh(pos, vel, boundary, reserve=n + 8 * 4096)
    ctx.profile_enable(True)
    wall, dev = timed(ctx, args.calls, lambda: ctx.upload(pos, vel), lambda: ctx.append(extra))
    out["append_4096_in_place"] = dict(wall_us=wall, by_label_us=dev)
    ctx.close()
    walls = []
    for _ in range(max(3, args.calls // 3)):
        ctx = fresh(pos, vel, boundary)
        ctx.synchronize()
        t0 = time.perf_counter()
        ctx.append(extra)
        walls.append((time.perf_counter() - t0) * 1e6)
        ctx.close()
    out["append_4096_with_growth"] = dict(wall_us=float(np.median(walls)))
    line = json.dumps(out)
    print(line)
    path = args.out or os.path.join(ROOT, "profiles", "edit", "edit_%d.json" % args.particles)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
