#!/usr/bin/env python3
"""Cost of editing the particle set on the device (sphx_remove / sphx_append) next to the round trip they replace.

  tools/edit_bench.py [--particles 1000000] [--warmup 50] [--calls 9] [--tiles K] [--tiles-only] [--out profiles/edit/edit_<n>.json]

The dam-break scene is stepped --warmup times; on that state, --calls times each (the state is put back by a fresh upload of the same
arrays in between, so every call sees the same particles):
  * sphx_remove with 0 %, 1 % and 50 % removed (a half plane x >= the matching quantile of the positions);
  * sphx_append of 4096 particles into reserved room (in place) and into exact capacity (the arrays grow by half);
  * the round trip: download + numpy filter (1 % removed) + upload.
Per case: the median wall time of the call (us; it includes the call's one synchronisation), the device time of its launches by label
(sphx_profile_*, median per call), and for sphx_remove the achieved bandwidth against the byte model 8 B per particle read for the
predicate + 40 B per survivor moved (nothing is moved when nothing goes).  Prints one JSON line and writes it to --out.

--tiles K adds the edits of a tiled run (sphx_multi_remove / sphx_multi_append) on K in-process tiles of device 0, after the same warm-up
(--tiles-only: nothing else; the file is then edit_multi_<n>_<K>.json).  Every call starts from the same state, put back by
sphx_multi_state_load of a part saved after the warm-up:
  * sphx_multi_remove with 0 %, 1 % and 50 % removed: wall time of the call, and per tile the two launches of the marking pass from the
    library's hipEvent brackets (tile_remove_mark, tile_remove_scan) with the mark pass's bandwidth against its byte model, 12 B per local
    record + 4 B per removed one + 4 B per workgroup;
  * sphx_multi_append of 4096 records in place, and of as many records as overflow one tile's reserve (the arrays grow);
  * the round trip sphx_multi_download + numpy filter (1 % removed) + sphx_multi_upload, and its ratio to sphx_multi_remove at 1 %."""
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


def bench_tiles(args):
    """sphx_multi_remove / sphx_multi_append on args.tiles in-process tiles: wall time of the calls, the marking pass per tile"""
    from yasph2d_amd.multi import MultiSolver

    K = args.tiles
    w = y.FluidParticleWorld()
    w.reset_fluid(float(np.sqrt(args.particles / 4050.0)))
    m = MultiSolver(y.default_params(), devices=[0] * K)
    m.set_boundary(w.boundary_particles)
    m.upload(w.positions)
    m.steps(y.TimeManager(), args.warmup)
    blob = m.save_state()
    d0 = m.download()
    n = len(d0["ids"])
    xs = np.sort(d0["pos"][:, 0])
    ctxs = [m.tile_context(k) for k in range(K)]
    marks = ("tile_remove_mark", "tile_remove_scan")
    out = dict(tiles=K, particles=n, info={k: v for k, v in m.info().items() if k in ("cap_records", "peers", "halo_now", "grid_layout")})

    def wall_of(calls, fn, restore=True):
        ts = []
        for _ in range(calls):
            if restore:
                m.load_state(blob)
            m.synchronize()
            t0 = time.perf_counter()
            fn()
            m.synchronize()
            ts.append((time.perf_counter() - t0) * 1e6)
        return float(np.median(ts))

    for name, frac in (("remove_0pct", 0.0), ("remove_1pct", 0.01), ("remove_50pct", 0.5)):
        x0 = INF if frac == 0.0 else float(xs[n - int(round(frac * n))])
        removed = []
        wall = wall_of(args.calls, lambda: removed.append(m.remove((x0, -INF, INF, INF))))
        # the marking pass alone, bracketed by events, on the restored state (one call per restore: a second one would find nothing)
        per_tile = [dict(tile=k, mark_us=[], scan_us=[]) for k in range(K)]
        for _ in range(max(3, args.calls // 3)):
            m.load_state(blob)
            m.synchronize()
            for c in ctxs:
                c.profile_enable(True)
                c.profile_reset()
            m.remove((x0, -INF, INF, INF))
            m.synchronize()
            for k, c in enumerate(ctxs):
                prof = c.profile_get()
                for lab, key in zip(marks, ("mark_us", "scan_us")):
                    if lab in prof:
                        per_tile[k][key].append(1e3 * prof[lab]["total_ms"] / max(prof[lab]["launches"], 1))
                c.profile_enable(False)
        m.load_state(blob)
        for k, c in enumerate(ctxs):
            t = c.download(vel=False, density=False)
            own = (t["ids"] >> 31) == 1
            hits = int((own & (t["pos"][:, 0] >= np.float32(x0))).sum())
            row = per_tile[k]
            row.update(n_local=len(own), owned=int(own.sum()), removed=hits)
            row["mark_us"] = float(np.median(row["mark_us"])) if row["mark_us"] else None
            row["scan_us"] = float(np.median(row["scan_us"])) if row["scan_us"] else None
            row["model_bytes"] = 12.0 * len(own) + 4.0 * hits + 4.0 * ((len(own) + 255) // 256)
            if row["mark_us"]:
                row["mark_TB_per_s"] = row["model_bytes"] / (row["mark_us"] * 1e-6) / 1e12
        out[name] = dict(removed=removed[-1], wall_us=wall, per_tile=per_tile)

    x1 = float(xs[n - int(round(0.01 * n))])

    def round_trip():
        t = m.download()
        keep = ~(t["pos"][:, 0] >= np.float32(x1))
        m.upload(t["pos"][keep], t["vel"][keep])

    out["round_trip_1pct"] = dict(wall_us=wall_of(max(3, args.calls // 3), round_trip))
    out["round_trip_over_remove_1pct"] = out["round_trip_1pct"]["wall_us"] / out["remove_1pct"]["wall_us"]
    extra = (d0["pos"][:4096] + np.float32(0.001)).astype(np.float32)
    out["append_4096_in_place"] = dict(wall_us=wall_of(args.calls, lambda: m.append(extra)))
    # more records than one tile's reserve leaves room for (1.25 x owned + 2 max(2, peers) cap_records + 4 096 slots)
    m.load_state(blob)
    info = m.info()
    many = int(0.25 * max(len(c.download(pos=False, vel=False, density=False)["ids"]) for c in ctxs) + 2 * max(2, info["peers"]) * info["cap_records"] + 4096) + 4096
    g = np.stack(np.meshgrid(np.arange(270), np.arange(many // 270 + 1)), -1).reshape(-1, 2)[:many].astype(np.float32)
    hi = d0["pos"].max(0)  # a block at the fluid's own spacing in the air right of the column, its top at the column's: the upper right tile's
    big = (np.float32([hi[0] + 1.0, hi[1] - (many // 270 + 1) / 90.0]) + g * np.float32(1.0 / 90.0)).astype(np.float32)
    out["append_with_growth"] = dict(records=many, wall_us=wall_of(max(3, args.calls // 3), lambda: m.append(big)))
    m.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", type=int, default=1_000_000)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--calls", type=int, default=9)
    ap.add_argument("--tiles", type=int, default=0, help="also measure sphx_multi_remove / sphx_multi_append on this many in-process tiles of device 0")
    ap.add_argument("--tiles-only", action="store_true", help="with --tiles: skip the single context")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.tiles and args.tiles_only:
        line = json.dumps(dict(warmup=args.warmup, calls=args.calls, multi=bench_tiles(args)))
        print(line)
        path = args.out or os.path.join(ROOT, "profiles", "edit", "edit_multi_%d_%d.json" % (args.particles, args.tiles))
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as f:
            f.write(line + "\n")
        return
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
    if args.tiles:
        out["multi"] = bench_tiles(args)
    line = json.dumps(out)
    print(line)
    path = args.out or os.path.join(ROOT, "profiles", "edit", "edit_%d.json" % args.particles)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
