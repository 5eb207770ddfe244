#!/usr/bin/env python3
"""Cost of rendering a frame on the device (sphx_render) on the bench scene (the 16 M dam break), next to what a user could do before.

  tools/render_bench.py [--particles 16000000] [--warmup 40] [--steps 40] [--calls 25]
  tools/render_bench.py --tiles K [--particles 16000000] [--warmup 10] [--calls 25]

As tools/sample_bench.py: a scratch context keeps the GPU busy until the context's first step is queued, then --warmup untimed steps
settle the flow.  Measured on that settled state, all in this one process, medians of --calls calls:
  * A: the whole scene (the app's camera, main.rs:137, times the scene scale) at 1920 x 1080 with min_pixel_radius = 0.75;
  * B: the same frame with the reference's radius (min_pixel_radius = 0);
  * C: 1920 x 1080 zoomed so that a disc is 6 pixels wide (pixel_per_world_unit = 3 / particle_radius), centred on the median particle;
    each as kernel time (the hipEvent brackets of the call's launches: clear, scatter over the boundary, scatter over the fluid, resolve;
    device-pointer path, rgba only) and as host-path wall time (rgba into host memory);
  * the viewer feed: sphx_view_request(1) + sphx_view_fetch(wait) (12 bytes per particle to the host), wall time;
  * sphx_sample_grid of the velocity on a 1920 x 1080 lattice over the domain's box: kernel time and host-path wall time.
--tiles K is the tiled run's picture (sphx_multi_render): the same scene in a single context and in a K-tile sphx_multi with all tiles on
device 0 (devices=[0] * K: the tiles' passes SERIALISE on the one GPU, and nothing here says anything about links), --warmup steps
each; views A, B and C as above on both: the kernels' time (single: clear, scatter, resolve; tiled: every tile's clear, scatter and layer
resolve over its window, summed over the tiles) and the host-path wall time (rgba alone, rgba + owner); the tiles' windows in pixels;
and sphx_multi_download of that run, the path the tiled picture replaces.
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
from tools.sample_bench import busy, scene  # noqa: E402

LABELS = ("render_clear", "render_scatter", "render_resolve")


TILE_LABELS = ("render_clear", "render_scatter_tile", "render_resolve_layer")


def wall_us(calls, f):
    out = []
    for _ in range(calls):
        t0 = time.perf_counter()
        f()
        out.append((time.perf_counter() - t0) * 1e6)
    return float(np.median(out))


def tiled(args):
    import ctypes as C

    import torch

    from yasph2d_amd import _lib
    from yasph2d_amd.multi import MultiSolver

    scale = float(np.sqrt(args.particles / 4050.0))
    whole = tuple(v * scale for v in y.SCENE_RECT)
    out = dict(tiles=args.tiles, warmup=args.warmup, calls=args.calls)

    def views_of(pos, radius):
        median = (float(np.median(pos[:, 0])), float(np.median(pos[:, 1])))
        return dict(A_whole_min_pixel_radius=y.render_fit(1920, 1080, whole, min_pixel_radius=0.75), B_whole_reference_radius=y.render_fit(1920, 1080, whole),
                    C_zoom_6_pixel_discs=y.render_fit(1920, 1080, whole, center=median, pixel_per_world_unit=3.0 / radius))

    # the single context holding the scene
    w = scene(args.particles)
    radius = float(w.properties()["particle_radius"])
    s = y.DFSPHSolver(w, y.default_params())
    t = y.TimeManager()
    s.simulation_steps(w, t, args.warmup, sync_world=False)
    ctx = s.context()
    ctx.synchronize()
    out["particles"], out["boundary"] = ctx.n, ctx.nb
    views = views_of(ctx.download(vel=False, density=False, ids=False)["pos"], radius)
    img = torch.empty((1080, 1920, 4), dtype=torch.uint8, device="cuda")
    single = {}
    for name, view in views.items():
        ctx.profile_filter(None)
        ctx.profile_enable(True)
        dev = []
        for _ in range(args.calls):
            ctx.profile_reset()
            ctx.render(view, out=img)
            p = ctx.profile_get()
            dev.append(sum(p[k]["total_ms"] for k in LABELS) * 1e3)
        ctx.profile_enable(False)
        single[name] = dict(kernels_us=float(np.median(dev)), host_rgba_us=wall_us(args.calls, lambda: ctx.render(view)),
                            host_rgba_owner_us=wall_us(args.calls, lambda: ctx.render(view, owner=True)))
    out["single"] = single
    del img
    s.close()

    # the same scene cut into tiles, all on device 0
    w = scene(args.particles)
    m = MultiSolver(y.default_params(), devices=[0] * args.tiles)
    m.set_boundary(w.boundary_particles)
    m.upload(w.positions)
    t = y.TimeManager()
    m.steps(t, args.warmup)
    m.synchronize()
    tcs = [m.tile_context(k) for k in range(args.tiles)]
    out["n_local_per_tile"] = [tc.n for tc in tcs]
    multi = {}
    for name, view in views.items():
        for tc in tcs:
            tc.profile_filter(None)
            tc.profile_enable(True)
        # (one tile after the other, each waited for: brackets of passes that run side by side on one GPU would count the waiting twice)
        dev, parts, wins = [], {k: [] for k in TILE_LABELS}, []
        for _ in range(args.calls):
            tot, wins = {k: 0.0 for k in TILE_LABELS}, []
            for tc in tcs:
                win, lay = (C.c_uint32 * 4)(), _lib.SphxRenderLayer()
                tc.profile_reset()
                tc._chk(m.L.sphx_tile_render_window(tc.h, C.byref(view), 1, win, C.byref(lay)))
                tc.synchronize()
                p = tc.profile_get()
                for k in TILE_LABELS:
                    tot[k] += p[k]["total_ms"] * 1e3 if k in p else 0.0
                wins.append((win[1] - win[0]) * (win[3] - win[2]))
            dev.append(sum(tot.values()))
            for k in TILE_LABELS:
                parts[k].append(tot[k])
        for tc in tcs:
            tc.profile_enable(False)
        img, own = m.render(view, owner=True)
        fluid = own < _lib.RENDER_BOUNDARY
        multi[name] = dict(kernels_us_all_tiles=float(np.median(dev)), parts_us={k: float(np.median(v)) for k, v in parts.items()},
                           host_rgba_us=wall_us(args.calls, lambda: m.render(view)), host_rgba_owner_us=wall_us(args.calls, lambda: m.render(view, owner=True)),
                           window_pixels_per_tile=wins, window_pixels_over_frame=sum(wins) / (1920.0 * 1080.0), fluid_pixels=int(fluid.sum()),
                           boundary_pixels=int((own == _lib.RENDER_BOUNDARY).sum()))
    out["multi"] = multi
    calls = max(3, args.calls // 5)
    out["multi_download"] = dict(bytes=24 * int(m.L.sphx_multi_num_owned(m.h)), host_us=wall_us(calls, m.download), calls=calls)
    for name in views:
        out["kernels_ratio_%s" % name[0]] = multi[name]["kernels_us_all_tiles"] / single[name]["kernels_us"]
        out["host_rgba_ratio_%s" % name[0]] = multi[name]["host_rgba_us"] / single[name]["host_rgba_us"]
    m.close()
    print(json.dumps(out))


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", type=int, default=16_000_000)
    ap.add_argument("--warmup", type=int, default=None)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--calls", type=int, default=25)
    ap.add_argument("--tiles", type=int, default=0, help="the tiled run's picture on K tiles of device 0, next to the single context's")
    args = ap.parse_args()
    if args.warmup is None:
        args.warmup = 10 if args.tiles else 40
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
    s.simulation_steps(w, t, args.steps, sync_world=False)
    ctx.synchronize()
    ms_step = (time.perf_counter() - t0) * 1e3 / args.steps
    n, nb = ctx.n, ctx.nb
    out = dict(particles=n, boundary=nb, scale=scale, warmup=args.warmup, steps=args.steps, calls=args.calls, ms_per_step=ms_step)
    pos = ctx.download(vel=False, density=False, ids=False)["pos"]
    median = (float(np.median(pos[:, 0])), float(np.median(pos[:, 1])))
    whole = tuple(v * scale for v in y.SCENE_RECT)
    views = dict(A_whole_min_pixel_radius=y.render_fit(1920, 1080, whole, min_pixel_radius=0.75), B_whole_reference_radius=y.render_fit(1920, 1080, whole),
                 C_zoom_6_pixel_discs=y.render_fit(1920, 1080, whole, center=median, pixel_per_world_unit=3.0 / radius))
    ctx.profile_reset()
    ctx.profile_filter(None)
    ctx.profile_enable(True)
    out["event_overhead_us"] = ctx.profile_event_overhead() * 1e3
    img = torch.empty((1080, 1920, 4), dtype=torch.uint8, device="cuda")
    for name, view in views.items():
        dev, parts, wall = [], {k: [] for k in LABELS}, []
        for _ in range(args.calls):
            ctx.profile_reset()
            ctx.render(view, out=img)
            p = ctx.profile_get()
            dev.append(sum(p[k]["total_ms"] for k in LABELS) * 1e3)
            for k in LABELS:
                parts[k].append(p[k]["total_ms"] * 1e3)
        ctx.profile_enable(False)
        for _ in range(args.calls):
            t0 = time.perf_counter()
            host = ctx.render(view, owner=True)
            wall.append((time.perf_counter() - t0) * 1e6)
        ctx.profile_enable(True)
        own = host[1]
        fluid = own < y._lib.RENDER_BOUNDARY
        out[name] = dict(pixel_per_world_unit=float(view.pixel_per_world_unit), kernels_us=float(np.median(dev)),
                         parts_us={k: float(np.median(v)) for k, v in parts.items()}, host_rgba_owner_us=float(np.median(wall)),
                         fluid_pixels=int(fluid.sum()), boundary_pixels=int((own == y._lib.RENDER_BOUNDARY).sum()),
                         particles_owning_a_pixel=int(len(np.unique(own[fluid]))))
        wall = []
        for _ in range(args.calls):
            t0 = time.perf_counter()
            ctx.render(view)
            wall.append((time.perf_counter() - t0) * 1e6)
        out[name]["host_rgba_us"] = float(np.median(wall))
    # the viewer feed: every particle to the host
    ctx.profile_enable(False)
    wall = []
    for _ in range(args.calls):
        t0 = time.perf_counter()
        ctx.view_request(1)
        ctx.view_fetch(wait=True)
        wall.append((time.perf_counter() - t0) * 1e6)
    out["view_feed"] = dict(bytes=12 * n, host_us=float(np.median(wall)))
    # the velocity field on the same lattice size
    ctx.profile_enable(True)
    nx, ny = 1920, 1080
    dx, dy = np.float32(2.0 * scale / nx), np.float32(2.5 * scale / ny)
    dev, wall = [], []
    for _ in range(args.calls):
        ctx.profile_reset()
        t0 = time.perf_counter()
        ctx.sample_grid((np.float32(0), np.float32(0)), (dx, dy), (ny, nx), fields=("velocity",))
        wall.append((time.perf_counter() - t0) * 1e6)
        dev.append(ctx.profile_get()["sample_grid"]["total_ms"] * 1e3)
    out["sample_grid_velocity"] = dict(kernel_us=float(np.median(dev)), host_us=float(np.median(wall)))
    ctx.profile_enable(False)
    s.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
