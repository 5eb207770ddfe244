#!/usr/bin/env python3
"""Cost of the per-particle flow fields (sphx_particle_fields) on the bench scene (the 16 M dam break), next to the walk they are modelled
on: the step's non-pressure pass (k_nonpressure<XSPH>, label nonpressure_accel_vmax), measured in the same run.

  tools/fields_bench.py [--particles 16000000] [--warmup 40] [--steps 40] [--calls 25] [--tiles K]

As tools/sample_bench.py: a scratch context keeps the GPU busy until the context's first step is queued, then --warmup untimed steps
settle the flow.  Measured on that settled state:
  * ms per step over --steps steps, and the non-pressure pass's time per launch (sphx_profile_*, every launch of its label);
  * all outputs, the velocity-gradient outputs only and the colour gradient only on the device-pointer path (torch outputs): device time
    per call = the hipEvent bracket of its one launch, median of --calls calls;
  * the host path's wall time for all outputs (the 32 bytes per particle cross to the host), median of --calls calls.
The estimate stated before the measurement: all outputs cost at most 1.5 x the non-pressure pass (the same staged record, walked over
count_total instead of count_dynamic entries, 32 bytes written per particle instead of 8).  Prints one JSON line.
--tiles K measures the tiled call instead (sphx_multi_particle_fields, K tiles on device 0) after warmup + steps + steps steps: per call
the host wall time, the device time of count + scan and of the walks summed over the tiles (sphx_profile_* of the tile contexts) and the
bytes that come back.  The expectation: at K = 1 the walk costs what k_particle_fields costs plus a 4-byte id
read per particle, and the count + scan on top."""
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

ESTIMATE = 1.5
NONPRESSURE = "nonpressure_accel_vmax"
SHAPE = dict(vel_grad=(2, 2), divergence=(), vorticity=(), color_grad=(2,))


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


def timed(ctx, calls, fn):
    """median device time (us) of the one launch per call, and median wall time (us) of the call"""
    dev, wall = [], []
    for _ in range(calls):
        ctx.profile_reset()
        t0 = time.perf_counter()
        fn()
        wall.append((time.perf_counter() - t0) * 1e6)
        ctx.synchronize()
        p = ctx.profile_get()["particle_fields"]
        assert p["launches"] == 1
        dev.append(p["total_ms"] * 1e3)
    return float(np.median(dev)), float(np.median(wall))


COUNT_SCAN = ("tile_fields_count", "tile_fields_scan")
WALK = "tile_particle_fields"


def tiled(args):
    """sphx_multi_particle_fields on K tiles of device 0 after warmup + steps + steps steps: per call (medians of --calls calls) the
    host wall time, the device time of count + scan (both rounds: the capacity check and the queued pass) and of the walks, summed over
    the tiles, and the bytes that come back; next to the wall time of the sphx_multi_download a second context would start from"""
    from yasph2d_amd.multi import MultiSolver

    w = scene(args.particles)
    m = MultiSolver(y.default_params(), devices=[0] * args.tiles)
    m.set_boundary(w.boundary_particles)
    m.upload(np.ascontiguousarray(w.positions, np.float32))
    t = y.TimeManager()
    m.steps(t, args.warmup)
    m.synchronize()
    t0 = time.perf_counter()
    m.steps(t, args.steps)
    m.synchronize()
    ms_step = (time.perf_counter() - t0) * 1e3 / args.steps
    m.steps(t, args.steps)
    m.synchronize()
    tiles = [m.tile_context(k) for k in range(args.tiles)]
    local = [c.n for c in tiles]
    before = m.info()["exchanges"]
    n = len(m.fields("divergence")["ids"])  # (grows the scratch; refreshes a spent band once)
    out = dict(particles=n, tiles=args.tiles, warmup=args.warmup, steps=args.steps, calls=args.calls, ms_per_step=ms_step, local_particles=local,
               ghost_fraction=float(sum(local) - n) / max(sum(local), 1), ghost_rings=m.ghost_rings())
    sets = (("all_outputs", tuple(SHAPE), 32), ("velocity_gradient_only", ("vel_grad", "divergence", "vorticity"), 24), ("color_grad_only", ("color_grad",), 8))
    for name, fields, _ in sets:  # pass 1, profiler off: the wall time of the whole host call
        m.fields(fields)
        wall = []
        for _ in range(args.calls):
            t0 = time.perf_counter()
            m.fields(fields)
            wall.append((time.perf_counter() - t0) * 1e6)
        out[name] = dict(call_wall_us=float(np.median(wall)))
    for c in tiles:  # pass 2, profiler on: the device time of every tile's launches
        c.profile_reset()
        c.profile_filter(None)
        c.profile_enable(True)
    for name, fields, width in sets:
        cs, walk = [], []
        for _ in range(args.calls):
            for c in tiles:
                c.profile_reset()
            m.fields(fields)
            m.synchronize()
            prof = [c.profile_get() for c in tiles]
            cs.append(sum(p[lab]["total_ms"] * 1e3 for p in prof for lab in COUNT_SCAN if lab in p))
            walk.append(sum(p[WALK]["total_ms"] * 1e3 for p in prof if WALK in p))
        out[name].update(count_scan_us=float(np.median(cs)), walk_us=float(np.median(walk)), bytes_back=(width + 4) * n,
                         particles_per_s=n / (float(np.median(walk)) * 1e-6))
    for c in tiles:
        c.profile_enable(False)
    wall = []
    for _ in range(max(3, args.calls // 5)):
        t0 = time.perf_counter()
        m.download()
        wall.append((time.perf_counter() - t0) * 1e6)
    out["multi_download_us"] = float(np.median(wall))
    out["exchanges_caused"] = m.info()["exchanges"] - before
    m.close()
    print(json.dumps(out))


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", type=int, default=16_000_000)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--calls", type=int, default=25)
    ap.add_argument("--tiles", type=int, default=0, help="measure sphx_multi_particle_fields on this many tiles of device 0 instead")
    args = ap.parse_args()
    if args.tiles:
        tiled(args)
        return
    stop = threading.Event()
    th = threading.Thread(target=busy, args=(stop, args.particles), daemon=True)
    th.start()
    time.sleep(0.3)
    w = scene(args.particles)
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
    p = ctx.profile_get()[NONPRESSURE]
    nonp_us = p["total_ms"] * 1e3 / p["launches"]
    n = ctx.n
    out = dict(particles=n, warmup=args.warmup, steps=args.steps, calls=args.calls, ms_per_step=ms_step,
               density_iterations=float(np.mean([x["density_iterations"] for x in st])),
               divergence_iterations=float(np.mean([x["divergence_iterations"] for x in st])),
               neighbor_entries_per_particle=st[-1]["neighbor_entries"] / n,
               nonpressure=dict(label=NONPRESSURE, us=nonp_us, launches=p["launches"]), event_overhead_us=ctx.profile_event_overhead() * 1e3,
               estimate_ratio_all_outputs=ESTIMATE)
    bufs = {f: torch.empty((n,) + SHAPE[f], dtype=torch.float32, device="cuda") for f in SHAPE}
    for name, fields in (("all_outputs", tuple(SHAPE)), ("velocity_gradient_only", ("vel_grad", "divergence", "vorticity")), ("color_grad_only", ("color_grad",))):
        sub = {f: bufs[f] for f in fields}
        us, wall = timed(ctx, args.calls, lambda: ctx.fields(out=sub))
        out[name] = dict(us=us, ratio_to_nonpressure=us / nonp_us, particles_per_s=n / (us * 1e-6), call_wall_us=wall, step_fraction=us * 1e-3 / ms_step)
    us, wall = timed(ctx, args.calls, lambda: ctx.fields())
    out["host_path_all_outputs"] = dict(kernel_us=us, call_wall_us=wall, bytes=32 * n)
    out["estimate_holds"] = bool(out["all_outputs"]["ratio_to_nonpressure"] <= ESTIMATE)
    ctx.profile_enable(False)
    s.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
