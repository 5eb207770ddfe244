#!/usr/bin/env python3
"""Cost of rendering a frame on the device (sphx_render) on the bench scene (the 16 M dam break), next to what a user could do before.

  tools/render_bench.py [--particles 16000000] [--warmup 40] [--steps 40] [--calls 25]

As tools/sample_bench.py: a scratch context keeps the GPU busy until the context's first step is queued, then --warmup untimed steps
settle the flow.  Measured on that settled state, all in this one process, medians of --calls calls:
  * A: the whole scene (the app's camera, main.rs:137, times the scene scale) at 1920 x 1080 with min_pixel_radius = 0.75;
  * B: the same frame with the reference's radius (min_pixel_radius = 0);
  * C: 1920 x 1080 zoomed so that a disc is 6 pixels wide (pixel_per_world_unit = 3 / particle_radius), centred on the median particle;
    each as kernel time (the hipEvent brackets of the call's launches: clear, scatter over the boundary, scatter over the fluid, resolve;
    device-pointer path, rgba only) and as host-path wall time (rgba into host memory);
  * the viewer feed: sphx_view_request(1) + sphx_view_fetch(wait) (12 bytes per particle to the host), wall time;
  * sphx_sample_grid of the velocity on a 1920 x 1080 lattice over the domain's box: kernel time and host-path wall time.
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


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", type=int, default=16_000_000)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--calls", type=int, default=25)
    args = ap.parse_args()
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
