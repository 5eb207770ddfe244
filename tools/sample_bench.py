#!/usr/bin/env python3
"""Cost of field sampling (sphx_sample_points / sphx_sample_grid) on the bench scene (the 16 M dam break), next to the step it reads.

  tools/sample_bench.py [--particles 16000000] [--warmup 40] [--steps 40] [--calls 25] [--tiles K]

As tools/viscosity_ab.py: a scratch context keeps the GPU busy until the context's first step is queued, then --warmup untimed
steps settle the flow.  Measured on that settled state:
  * ms per step over --steps steps, and the neighbour build's time per launch (sphx_profile_*, every launch of the build's labels);
  * A, frame: a 1920 x 1080 lattice over the domain's box [0, 2s] x [0, 2.5s] (s = scene scale), density + fraction + velocity;
  * B, particle spacing: a lattice at spacing 2 * particle_radius over the fluid's bounding box (about one point per particle),
    density + fraction + velocity;
  * C, 1 M random points: uniform in the fluid's bounding box, in random order and then sorted by cell (Morton order of the cell of
    cell_of) on the host, density + fraction + velocity.
Each configuration is called --calls times; device time per call = the hipEvent bracket of its one launch (median), minus nothing (the
bracket's own cost is printed as event_overhead_us).  C also reports the host-path wall time of the whole call (copies included).
--tiles K measures the tiled calls instead (sphx_multi_sample_grid / _points, K tiles on device 0): the frame of A and 2^20 points
sorted by cell, as wall time of the whole host call (median, profiler off) and, in a second pass, as the device time of every tile's
launches (sphx_profile_* of the tile contexts), next to the wall time of the sphx_multi_download the calls replace and the halo exchanges they caused.
Prints one JSON line."""
import argparse
import json
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import yasph2d_amd as y  # noqa: E402

FIELDS = ("density", "fraction", "velocity")


def scene(n):
    w = y.FluidParticleWorld()
    w.reset_fluid(float(np.sqrt(n / 4050.0)))
    return w


def busy(stop, n):
    w = scene(min(n, 16_000_000))
    s = y.DFSPHSolver(w, y.default_params())
    t = y.TimeManager()
    while not stop.is_set():
        s.simulation_steps(w, t, 4, sync_world=False)
    s.close()


def part1by1(x):
    x = x.astype(np.uint64) & 0xFFFF
    x = (x ^ (x << 8)) & 0x00FF00FF
    x = (x ^ (x << 4)) & 0x0F0F0F0F
    x = (x ^ (x << 2)) & 0x33333333
    x = (x ^ (x << 1)) & 0x55555555
    return x


def timed(ctx, label, calls, fn):
    """median device time (us) of the one launch per call, and median wall time (us) of the call"""
    dev, wall = [], []
    for _ in range(calls):
        ctx.profile_reset()
        t0 = time.perf_counter()
        fn()
        wall.append((time.perf_counter() - t0) * 1e6)
        ctx.synchronize()
        p = ctx.profile_get()[label]
        assert p["launches"] == 1
        dev.append(p["total_ms"] * 1e3)
    return float(np.median(dev)), float(np.median(wall)), dev


def wall_us(calls, fn):
    out = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e6)
    return float(np.median(out))


def tiled(args):
    """the tiled calls on K tiles of device 0: host wall time per call, device time per tile and pass, the download they replace"""
    from yasph2d_amd.multi import MultiSolver

    scale = float(np.sqrt(args.particles / 4050.0))
    w = scene(args.particles)
    pos = np.ascontiguousarray(w.positions, np.float32)
    p = y.default_params()
    m = MultiSolver(p, devices=[0] * args.tiles)
    m.set_boundary(w.boundary_particles)
    m.upload(pos)
    t = y.TimeManager()
    m.steps(t, args.warmup)
    m.synchronize()
    t0 = time.perf_counter()
    m.steps(t, args.steps)
    m.synchronize()
    ms_step = (time.perf_counter() - t0) * 1e3 / args.steps
    tiles = [m.tile_context(k) for k in range(args.tiles)]
    n = int(m.info()["owned_local"])
    out = dict(particles=n, tiles=args.tiles, scale=scale, warmup=args.warmup, steps=args.steps, calls=args.calls, ms_per_step=ms_step,
               ghost_rings=m.ghost_rings(), tile_rects=m.tile_rects().tolist())
    d = m.download()
    lo, hi = d["pos"].min(0), d["pos"].max(0)
    out["multi_download_us"] = wall_us(max(3, args.calls // 5), m.download)
    nx, ny = 1920, 1080
    dx, dy = np.float32(2.0 * scale / nx), np.float32(2.5 * scale / ny)
    rng = np.random.default_rng(1)
    k = 1 << 20
    pts = (lo + rng.random((k, 2), dtype=np.float32) * (hi - lo)).astype(np.float32)
    cell = np.fmin(np.fmax((pts - np.array(p.grid_min[:], np.float32)) * np.float32(np.float32(1) / np.float32(p.smoothing_length)), 0), 65535).astype(np.uint32)
    pts = np.ascontiguousarray(pts[np.argsort((part1by1(cell[:, 1]) << np.uint64(1)) | part1by1(cell[:, 0]), kind="stable")])
    before = m.info()["exchanges"]
    queries = (("frame_1920x1080", lambda: m.sample_grid((np.float32(0), np.float32(0)), (dx, dy), (ny, nx), fields=FIELDS), ("tile_sample_window",)),
               ("points_2^20_sorted_by_cell", lambda: m.sample(pts, fields=FIELDS), ("tile_sample_select", "tile_sample_indexed")))
    # pass 1, profiler off: the wall time of the whole host call
    for name, fn, _ in queries:
        fn()  # (grows the scratch)
        out[name] = dict(host_call_us=wall_us(args.calls, fn))
    # pass 2, profiler on: the device time of every tile's launches (the hipEvent brackets would be inside pass 1's wall time)
    for c in tiles:
        c.profile_reset()
        c.profile_filter(None)
        c.profile_enable(True)
    for name, fn, labels in queries:
        for c in tiles:
            c.profile_reset()
        for _ in range(args.calls):
            fn()
        m.synchronize()
        per_tile = []
        for c in tiles:
            prof = c.profile_get()
            per_tile.append({lab: prof[lab]["total_ms"] * 1e3 / prof[lab]["launches"] for lab in labels if lab in prof and prof[lab]["launches"]})
        out[name].update(device_us_per_tile=per_tile, device_us_all_tiles=float(sum(sum(x.values()) for x in per_tile)))
    for c in tiles:
        c.profile_enable(False)
    out["exchanges_caused"] = m.info()["exchanges"] - before
    m.close()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", type=int, default=16_000_000)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--calls", type=int, default=25)
    ap.add_argument("--tiles", type=int, default=0, help="measure sphx_multi_sample_* on this many tiles of device 0 instead")
    args = ap.parse_args()
    if args.tiles:
        return tiled(args)
    scale = float(np.sqrt(args.particles / 4050.0))
    stop = threading.Event()
    th = threading.Thread(target=busy, args=(stop, args.particles), daemon=True)
    th.start()
    time.sleep(0.3)
    w = scene(args.particles)
    radius = float(w.properties()["particle_radius"])
    s = y.DFSPHSolver(w, y.default_params())
    t = y.TimeManager()
    s.simulation_steps(w, t, 1, sync_world=False)  # the upload step, still under the scratch load
    stop.set()
    th.join()
    s.simulation_steps(w, t, args.warmup, sync_world=False)
    ctx = s.context()
    ctx.synchronize()
    t0 = time.perf_counter()
    st = s.simulation_steps(w, t, args.steps, sync_world=False)
    ctx.synchronize()
    ms_step = (time.perf_counter() - t0) * 1e3 / args.steps
    ctx.profile_reset()
    ctx.profile_filter(None)
    ctx.profile_enable(True)
    s.simulation_steps(w, t, args.steps, sync_world=False)
    ctx.synchronize()
    prof = ctx.profile_get()
    builds = {k: dict(us=v["total_ms"] * 1e3 / v["launches"], launches=v["launches"]) for k, v in prof.items() if k.startswith("neighbor_build")}
    main_build = max(builds, key=lambda k: builds[k]["launches"])
    n = ctx.n
    build_us = builds[main_build]["us"]
    out = dict(particles=n, scale=scale, warmup=args.warmup, steps=args.steps, calls=args.calls, ms_per_step=ms_step,
               density_iterations=float(np.mean([x["density_iterations"] for x in st])),
               divergence_iterations=float(np.mean([x["divergence_iterations"] for x in st])),
               neighbor_build=dict(label=main_build, us=build_us, particles_per_s=n / (build_us * 1e-6), all=builds),
               event_overhead_us=ctx.profile_event_overhead() * 1e3)
    d = ctx.download(vel=False, density=False, ids=False)
    pos = d["pos"]
    lo, hi = pos.min(0), pos.max(0)
    # A: the frame
    nx, ny = 1920, 1080
    dx, dy = np.float32(2.0 * scale / nx), np.float32(2.5 * scale / ny)
    us, wall, _ = timed(ctx, "sample_grid", args.calls, lambda: ctx.sample_grid((np.float32(0), np.float32(0)), (dx, dy), (ny, nx), fields=FIELDS))
    out["A_frame"] = dict(nx=nx, ny=ny, us=us, points_per_s=nx * ny / (us * 1e-6), host_call_us=wall, step_fraction=us * 1e-3 / ms_step)
    # B: particle spacing over the fluid's box
    sp = np.float32(2.0 * radius)
    bnx, bny = int(np.ceil((hi[0] - lo[0]) / sp)) + 1, int(np.ceil((hi[1] - lo[1]) / sp)) + 1
    us, wall, _ = timed(ctx, "sample_grid", args.calls, lambda: ctx.sample_grid((lo[0], lo[1]), (sp, sp), (bny, bnx), fields=FIELDS))
    pps = bnx * bny / (us * 1e-6)
    out["B_particle_spacing"] = dict(nx=bnx, ny=bny, points=bnx * bny, us=us, points_per_s=pps, host_call_us=wall,
                                     ratio_to_build_particles_per_s=pps / out["neighbor_build"]["particles_per_s"])
    # C: 1 M random points, random order and sorted by cell
    rng = np.random.default_rng(1)
    m = 1_000_000
    pts = (lo + rng.random((m, 2), dtype=np.float32) * (hi - lo)).astype(np.float32)
    p = y.default_params()  # (the parameters the solver was created with)
    cell = np.fmin(np.fmax((pts - np.array(p.grid_min[:], np.float32)) * np.float32(np.float32(1) / np.float32(p.smoothing_length)), 0), 65535).astype(np.uint32)
    order = np.argsort((part1by1(cell[:, 1]) << np.uint64(1)) | part1by1(cell[:, 0]), kind="stable")
    c = {}
    for name, q in (("random_order", pts), ("sorted_by_cell", np.ascontiguousarray(pts[order]))):
        us, wall, _ = timed(ctx, "sample_points", args.calls, lambda: ctx.sample(q, fields=FIELDS))
        c[name] = dict(us=us, points_per_s=m / (us * 1e-6), host_call_us=wall)
    c["random_over_sorted"] = c["random_order"]["us"] / c["sorted_by_cell"]["us"]
    out["C_1M_points"] = c
    ctx.profile_enable(False)
    # the wall time of the whole host call once more with the profiler off (what --tiles K reports as host_call_us)
    sorted_pts = np.ascontiguousarray(pts[order])
    out["A_frame"]["host_call_us_profiler_off"] = wall_us(args.calls, lambda: ctx.sample_grid((np.float32(0), np.float32(0)), (dx, dy), (ny, nx), fields=FIELDS))
    out["C_1M_points"]["sorted_by_cell"]["host_call_us_profiler_off"] = wall_us(args.calls, lambda: ctx.sample(sorted_pts, fields=FIELDS))
    s.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
