#!/usr/bin/env python3
"""Cost of the free-surface extraction (sphx_surface_contour, device-pointer mode) on the dam break, next to its two yardsticks.

  tools/contour_bench.py [--particles 16000000,1000000] [--warmup 40] [--calls 15] [--lattices 513x385,1025x769,1920x1080]

Per particle count: the scene is stepped --warmup times, then for every lattice (over the app's camera rectangle x scale):
  * the device time of every pass of sphx_surface_contour (sphx_profile_*: sample_grid = pass (a), contour_count, contour_carry,
    contour_emit; median over --calls calls with torch outputs on the device), and their sum;
  * yardstick 1: the device time of sphx_sample_grid(fraction) of the same lattice in device-pointer mode (the same kernel as pass (a));
  * yardstick 2, the route without the call: sphx_sample_grid into host memory (wall time, copy included) and marching squares in numpy
    (tests/contour_reference.py, wall time), measured twice;
  * the wall time of the whole host-pointer call (segments copied back) and of sphx_contour_chain on its segments.
Prints one JSON line per particle count.

  tools/contour_bench.py --tiles 1,2,4,8 [...]

The tiled call (sphx_multi_surface_contour) instead: per particle count and K the dam break runs as K tiles, all on device 0, and for
every lattice the tool reports per tile the device time of every pass (tile_sample_window, contour_border_pack, contour_apron_unpack,
contour_count, contour_carry, contour_emit; medians over --calls calls) and the wall time of the whole call, next to two yardsticks
measured in the same process on the same state: MultiSolver.sample_grid(fields=("fraction",)) (wall), and that plus contour32 in numpy —
the route the call replaces.  One JSON line per particle count and K."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import contour_reference as cr  # noqa: E402
import yasph2d_amd as y  # noqa: E402
from yasph2d_amd import _lib  # noqa: E402

PASSES = ("sample_grid", "contour_count", "contour_carry", "contour_emit")


def median_us(ctx, labels, calls, fn):
    per = {k: [] for k in labels}
    for _ in range(calls):
        ctx.profile_reset()
        fn()
        ctx.synchronize()
        p = ctx.profile_get()
        for k in labels:
            per[k].append(p[k]["total_ms"] * 1e3 if k in p else 0.0)
    return {k: float(np.median(v)) for k, v in per.items()}


def wall_us(calls, fn):
    out = []
    for _ in range(calls):
        t0 = time.perf_counter()
        r = fn()
        out.append((time.perf_counter() - t0) * 1e6)
    return float(np.median(out)), r


def run(n, args):
    import torch

    scale = float(np.sqrt(n / 4050.0))
    w = y.FluidParticleWorld()
    w.reset_fluid(scale)
    s = y.DFSPHSolver(w, y.default_params())
    t = y.TimeManager()
    s.simulation_steps(w, t, args.warmup, sync_world=False)
    ctx = s.context()
    ctx.synchronize()
    out = dict(particles=ctx.n, scale=scale, warmup=args.warmup, calls=args.calls, lattices=[])
    for spec in args.lattices.split(","):
        nx, ny = (int(v) for v in spec.split("x"))
        x0 = y0 = np.float32(-0.1 * scale)
        dx, dy = np.float32(2.2 * scale / (nx - 1)), np.float32(1.7 * scale / (ny - 1))
        count = ctx.contour((x0, y0), (dx, dy), (ny, nx), cap=0)["count"]
        cap = count + 16
        dev = dict(segments=torch.empty((cap, 4), device="cuda"), cell=torch.empty(cap, dtype=torch.int32, device="cuda"),
                   values=torch.empty((ny, nx), device="cuda"), count=torch.zeros(1, dtype=torch.int32, device="cuda"))
        frac = torch.empty((ny, nx), device="cuda")
        so = _lib.SphxSampleOut(fraction=frac.data_ptr())

        def sample_only():
            rc = ctx.L.sphx_sample_grid(ctx.h, x0, y0, dx, dy, nx, ny, y.KERNEL_WENDLAND_C2, _lib.SAMPLE_DEVICE_POINTERS, C.byref(so))
            assert rc == 0

        ctx.profile_filter(None)
        ctx.profile_enable(True)
        passes = median_us(ctx, PASSES, args.calls, lambda: ctx.contour((x0, y0), (dx, dy), (ny, nx), out=dev))
        yard1 = median_us(ctx, ("sample_grid",), args.calls, sample_only)["sample_grid"]
        ctx.profile_enable(False)
        total = sum(passes.values())
        extract = total - passes["sample_grid"]
        host_call, res = wall_us(max(3, args.calls // 5), lambda: ctx.contour((x0, y0), (dx, dy), (ny, nx), cap=cap))
        chain, lines = wall_us(3, lambda: y.contour_chain(res["segments"]))
        grid_wall, g = wall_us(2, lambda: ctx.sample_grid((x0, y0), (dx, dy), (ny, nx), fields=("fraction",))["fraction"])
        numpy_wall, ref = wall_us(2, lambda: cr.contour32(g, x0, y0, dx, dy, nx, ny, 0.5))
        assert ref["count"] == count and np.array_equal(ref["segments"].view(np.uint32), res["segments"].view(np.uint32))
        out["lattices"].append(dict(nx=nx, ny=ny, segments=count, lines=int(len(lines[2])), passes_us=passes, contour_us=total,
                                    passes_b_to_d_us=extract, b_to_d_over_a=extract / passes["sample_grid"],
                                    yardstick_sample_grid_us=yard1, contour_over_sample_grid=total / yard1,
                                    host_call_us=host_call, chain_us=chain,
                                    present_route=dict(sample_grid_host_us=grid_wall, numpy_marching_squares_us=numpy_wall,
                                                       total_us=grid_wall + numpy_wall, over_host_call=(grid_wall + numpy_wall) / host_call)))
    s.close()
    print(json.dumps(out), flush=True)


TILE_PASSES = ("tile_sample_window", "contour_border_pack", "contour_apron_unpack", "contour_count", "contour_carry", "contour_emit")


def run_tiles(n, k, args):
    scale = float(np.sqrt(n / 4050.0))
    w = y.FluidParticleWorld()
    w.reset_fluid(scale)
    s = y.DFSPHMultiSolver(w, [0] * k)
    t = y.TimeManager()
    s.simulation_steps(w, t, args.warmup, sync_world=False)
    m = s.multi()
    tiles = [m.tile_context(i) for i in range(k)]
    out = dict(particles=int(sum(c.n for c in tiles)), tiles=k, scale=scale, warmup=args.warmup, calls=args.calls, lattices=[])
    for spec in args.lattices.split(","):
        nx, ny = (int(v) for v in spec.split("x"))
        x0 = y0 = np.float32(-0.1 * scale)
        dx, dy = np.float32(2.2 * scale / (nx - 1)), np.float32(1.7 * scale / (ny - 1))
        count = m.contour((x0, y0), (dx, dy), (ny, nx), cap=0)["count"]
        cap = count + 16
        per = [{p: [] for p in TILE_PASSES} for _ in tiles]
        for c in tiles:
            c.profile_filter(None)
            c.profile_enable(True)
        for _ in range(args.calls):
            for c in tiles:
                c.profile_reset()
            m.contour((x0, y0), (dx, dy), (ny, nx), cap=cap)
            for i, c in enumerate(tiles):
                c.synchronize()
                prof = c.profile_get()
                for p in TILE_PASSES:
                    per[i][p].append(prof[p]["total_ms"] * 1e3 if p in prof else 0.0)
        for c in tiles:
            c.profile_enable(False)
        passes = [{p: float(np.median(v)) for p, v in one.items()} for one in per]
        call_wall, res = wall_us(args.calls, lambda: m.contour((x0, y0), (dx, dy), (ny, nx), cap=cap))
        count_wall, _ = wall_us(args.calls, lambda: m.contour((x0, y0), (dx, dy), (ny, nx), cap=0))
        grid_wall, g = wall_us(max(3, args.calls // 3), lambda: m.sample_grid((x0, y0), (dx, dy), (ny, nx), fields=("fraction",))["fraction"])
        numpy_wall, ref = wall_us(2, lambda: cr.contour32(g, x0, y0, dx, dy, nx, ny, 0.5))
        assert ref["count"] == count == res["count"] and np.array_equal(ref["segments"].view(np.uint32), res["segments"].view(np.uint32))
        out["lattices"].append(dict(nx=nx, ny=ny, segments=count, tile_passes_us=passes, tile_device_us=[sum(one.values()) for one in passes],
                                    call_wall_us=call_wall, count_only_wall_us=count_wall, yardstick_sample_grid_wall_us=grid_wall,
                                    yardstick_numpy_marching_squares_us=numpy_wall, present_route_us=grid_wall + numpy_wall,
                                    call_over_sample_grid=call_wall / grid_wall, present_route_over_call=(grid_wall + numpy_wall) / call_wall))
    s.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", default="16000000,1000000")
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--calls", type=int, default=15)
    ap.add_argument("--lattices", default="513x385,1025x769,1920x1080")
    ap.add_argument("--tiles", default=None, help="K1,K2,...: measure sphx_multi_surface_contour on K tiles (all on device 0) instead")
    args = ap.parse_args()
    for n in args.particles.split(","):
        if args.tiles:
            for k in args.tiles.split(","):
                run_tiles(int(n), int(k), args)
        else:
            run(int(n), args)


if __name__ == "__main__":
    main()
