#!/usr/bin/env python3
"""Cost of the fluid statistics (sphx_fluid_stats, sphx_stats_record) on the bench scene (the 16 M dam break), next to the existing
streaming pass over the same arrays: sphx_state_digest's kernel on the positions, velocities and densities (20 bytes per particle, as
stage 1 reads), measured in the same run.

  tools/stats_bench.py [--particles 16000000] [--warmup 40] [--steps 40] [--calls 25] [--rounds 3]
  rocprofv3 --kernel-trace --output-format csv -d DIR -- python3 tools/stats_bench.py --trace-run [--particles ...] [--calls 25]
  tools/stats_bench.py --from-trace DIR/.../*_kernel_trace.csv --particles N
  tools/stats_bench.py --tiles K [--particles 16000000] [--warmup 10] [--calls 25]

As tools/fields_bench.py: a scratch context keeps the GPU busy until the context's first step is queued, then --warmup untimed steps
settle the flow.  Without a profiler, on that settled state:
  * one call with 0 and with 8 rectangles on the device-pointer path: device time = the hipEvent brackets of its two launches
    (sphx_profile_*), median of --calls calls, and the wall time of the host-path call;
  * ms per step over --steps steps without and with an every = 1 recording, --rounds times in alternation: the recorder's cost as a
    percentage of the step.
--trace-run is the part a kernel trace is taken of (profiling slows the host: kernel times come from a run of their own): --calls times
sphx_state_digest, a call with 0 and a call with 8 rectangles.  --from-trace reads that trace: the digest kernel runs once per section,
in section order (an empty section has none), so launches 0, 1 and 3 of every call are the positions, velocities and densities; stage 1 alternates between 0 and 8
rectangles.  The ratio of a call's kernels to those three launches and the achieved bytes per second (20 bytes per particle) are
printed.  There is no pass / fail threshold.  Every mode prints one JSON line.
--tiles K is the tiled run's pass (sphx_multi_fluid_stats: stage 1 also streams particle_id and keeps the owned particles, 24 bytes per
particle): the same scene in a single context and in a K-tile sphx_multi with all tiles on device 0 (devices=[0]*K), --warmup steps each,
in one process; per tile the device time of a sphx_tile_fluid_stats call with 0 and with 8 rectangles by the same hipEvent brackets as the
single context's call, the ratio of tile 0's stage 1 to the single context's (K = 1: everything is owned, the ratio by bytes is 24 / 20)
and the wall time of the whole sphx_multi_fluid_stats call."""
import argparse
import csv
import json
import os
import re
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

INF = float("inf")
LABELS = ("stats_partial", "stats_combine")


def rects_for(scale):
    """eight probe rectangles on the dam break of this scale: one covers everything, one nothing, the others boxes of the fluid column"""
    s = float(scale)
    return [(-INF, -INF, INF, INF), (0.9 * s, 0.0, 0.1 * s, 2.0 * s), (0.0, 0.6 * s, 0.35 * s, 1.2 * s), (0.2 * s, 0.9 * s, 0.6 * s, 1.5 * s),
            (0.0, 0.7 * s, 2.0 * s, 0.75 * s), (1.0 * s, 0.0, 2.0 * s, 1.5 * s), (0.31 * s, 1.01 * s, 0.33 * s, 1.03 * s), (-INF, 0.95 * s, 0.4 * s, INF)]


def settled(args):
    import yasph2d_amd as y

    scale = float(np.sqrt(args.particles / 4050.0))

    def scene():
        w = y.FluidParticleWorld()
        w.reset_fluid(scale)
        return w

    def busy(stop):
        w = scene()
        s = y.DFSPHSolver(w, y.default_params())
        t = y.TimeManager()
        while not stop.is_set():
            s.simulation_steps(w, t, 4, sync_world=False)
        s.close()

    stop = threading.Event()
    th = threading.Thread(target=busy, args=(stop,), daemon=True)
    th.start()
    time.sleep(0.3)
    w = scene()
    s = y.DFSPHSolver(w, y.default_params())
    t = y.TimeManager()
    s.simulation_steps(w, t, 1, sync_world=False)  # the upload step, still under the scratch load
    stop.set()
    th.join()
    s.simulation_steps(w, t, args.warmup, sync_world=False)
    s.context().synchronize()
    return w, s, t, scale


def timed_call(ctx, calls, rects, out, call=None):
    dev, wall = [], []
    for _ in range(calls):
        ctx.profile_reset()
        t0 = time.perf_counter()
        if call is None:
            ctx.stats(rects, out=out)
        else:
            call(rects, out)
        wall.append((time.perf_counter() - t0) * 1e6)
        p = ctx.profile_get()
        assert all(p[k]["launches"] == 1 for k in LABELS)
        dev.append([p[k]["total_ms"] * 1e3 for k in LABELS])
    dev = np.median(np.array(dev), axis=0)
    return dict(stage1_us=float(dev[0]), stage2_us=float(dev[1]), us=float(dev.sum()), call_wall_us=float(np.median(wall)))


def measure(args):
    import torch

    w, s, t, scale = settled(args)
    ctx = s.context()
    n = ctx.n
    rects = rects_for(scale)
    out = dict(particles=n, warmup=args.warmup, steps=args.steps, calls=args.calls, rounds=args.rounds, bytes_per_particle=20)
    # the recorder's cost: the same steps without and with a frame behind each, in alternation
    off, on = [], []
    for _ in range(args.rounds):
        for rec, ms in ((0, off), (1, on)):
            ctx.stats_record(rects if args.record_rects else (), args.steps if rec else 0)
            ctx.synchronize()
            t0 = time.perf_counter()
            s.simulation_steps(w, t, args.steps, sync_world=False)
            ctx.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3 / args.steps)
    ctx.stats_record((), 0)
    out["recorder"] = dict(every=1, n_rects=len(rects) if args.record_rects else 0, ms_per_step_off=off, ms_per_step_on=on,
                           percent_over=100.0 * (float(np.median(on)) / float(np.median(off)) - 1.0))
    # one call, device-pointer path, by the hipEvent brackets of its launches
    ctx.profile_filter(None)
    ctx.profile_enable(True)
    out["event_overhead_us"] = ctx.profile_event_overhead() * 1e3
    buf = {k: torch.empty((1 + k) * 128, dtype=torch.uint8, device="cuda") for k in (0, 8)}
    for k in (0, 8):
        r = timed_call(ctx, args.calls, rects[:k], buf[k])
        r["bytes_per_s"] = 20.0 * n / (r["stage1_us"] * 1e-6)
        out["rects_%d" % k] = r
    ctx.profile_enable(False)
    wall = []
    for _ in range(args.calls):
        t0 = time.perf_counter()
        rec = ctx.stats(rects)
        wall.append((time.perf_counter() - t0) * 1e6)
    out["host_path_8_rects_wall_us"] = float(np.median(wall))
    out["counts"] = rec["count"].tolist()
    wall = []
    for _ in range(args.calls):
        t0 = time.perf_counter()
        ctx.state_digest()
        wall.append((time.perf_counter() - t0) * 1e6)
    out["state_digest_call_wall_us"] = float(np.median(wall))  # (all eight device sections, 44 bytes per particle, and the copy back)
    s.close()
    print(json.dumps(out))


def tiled(args):
    import torch

    import yasph2d_amd as y
    from yasph2d_amd import _lib
    from yasph2d_amd.multi import MultiSolver

    scale = float(np.sqrt(args.particles / 4050.0))
    w = y.FluidParticleWorld()
    w.reset_fluid(scale)
    rects = rects_for(scale)
    buf = {k: torch.empty((1 + k) * 128, dtype=torch.uint8, device="cuda") for k in (0, 8)}
    out = dict(particles=int(len(w.positions)), tiles=args.tiles, warmup=args.warmup, calls=args.calls)

    def brackets(ctx, n, bytes_pp, call=None):
        ctx.profile_filter(None)
        ctx.profile_enable(True)
        res = {}
        for k in (0, 8):
            r = timed_call(ctx, args.calls, rects[:k], buf[k], call)
            r["bytes_per_s"] = bytes_pp * n / (r["stage1_us"] * 1e-6) if n else 0.0
            res["rects_%d" % k] = r
        ctx.profile_enable(False)
        return res

    # the single context's pass (k_stats_partial<false>: 20 bytes per particle)
    s = y.DFSPHSolver(w, y.default_params())
    t = y.TimeManager()
    s.simulation_steps(w, t, args.warmup, sync_world=False)
    ctx = s.context()
    ctx.synchronize()
    out["single"] = dict(n=ctx.n, bytes_per_particle=20, **brackets(ctx, ctx.n, 20.0))
    s.close()

    # the same scene cut into tiles, all on device 0
    w = y.FluidParticleWorld()
    w.reset_fluid(scale)
    m = MultiSolver(y.default_params(), devices=[0] * args.tiles)
    m.set_boundary(w.boundary_particles)
    m.upload(w.positions)
    t = y.TimeManager()
    m.steps(t, args.warmup)
    m.synchronize()
    L = m.L
    per_tile = []
    for k in range(args.tiles):
        tc = m.tile_context(k)

        def call(r, o, tc=tc):
            arr, nr = y._rect_array(r)
            torch.cuda.current_stream().synchronize()
            tc._chk(L.sphx_tile_fluid_stats(tc.h, arr, nr, _lib.STATS_DEVICE_POINTERS, o.data_ptr()))
            tc.synchronize()

        per_tile.append(dict(tile=k, n_local=tc.n, bytes_per_particle=24, **brackets(tc, tc.n, 24.0, call)))
    out["tiles_detail"] = per_tile
    wall = []
    for _ in range(args.calls):
        t0 = time.perf_counter()
        rec, tiles = m.stats(rects, per_tile=True)
        wall.append((time.perf_counter() - t0) * 1e6)
    out["multi_call_8_rects_wall_us"] = float(np.median(wall))
    out["counts"] = rec["count"].tolist()
    out["owned_per_tile"] = tiles["count"][:, 0].tolist()
    for k in (0, 8):
        a, b = per_tile[0]["rects_%d" % k]["stage1_us"], out["single"]["rects_%d" % k]["stage1_us"]
        out["stage1_ratio_tile0_to_single_rects_%d" % k] = a / b
    out["byte_ratio"] = 24.0 / 20.0
    m.close()
    print(json.dumps(out))


def trace_run(args):
    import torch

    w, s, t, scale = settled(args)
    ctx = s.context()
    rects = rects_for(scale)
    buf = {k: torch.empty((1 + k) * 128, dtype=torch.uint8, device="cuda") for k in (0, 8)}
    for _ in range(args.calls):
        ctx.state_digest()
        ctx.stats((), out=buf[0])
        ctx.stats(rects, out=buf[8])
    print(json.dumps(dict(particles=ctx.n, calls=args.calls)))
    s.close()


def from_trace(args):
    rows = []
    with open(args.from_trace) as f:
        for r in csv.DictReader(f):
            k = re.sub(r"\(.*", "", r["Kernel_Name"]).replace("void ", "").replace("sphx::", "")
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), k))
    rows.sort()
    us = {k: [(e - b) * 1e-3 for b, e, name in rows if name.startswith(k)] for k in ("k_state_digest", "k_stats_partial", "k_stats_combine")}
    dig, p1, p2 = us["k_state_digest"], us["k_stats_partial"], us["k_stats_combine"]
    calls = len(p1) // 2
    assert calls and len(p1) == 2 * calls == len(p2) and len(dig) % calls == 0 and len(dig) // calls >= 4, (len(dig), len(p1), len(p2))
    per = len(dig) // calls  # (device sections that are not empty: a DFSPH run keeps no accelerations, 7 launches)
    three = [dig[i] + dig[i + 1] + dig[i + 3] for i in range(0, len(dig), per)]  # positions, velocities, densities
    n = args.particles
    out = dict(particles=n, calls=len(three), source="rocprofv3 --kernel-trace, a run of its own",
               digest_three_sections=dict(us=float(np.median(three)), bytes_per_s=20.0 * n / (float(np.median(three)) * 1e-6),
                                          launches_per_digest=per, positions_us=float(np.median(dig[0::per])), velocities_us=float(np.median(dig[1::per])),
                                          density_us=float(np.median(dig[3::per]))))
    for k, off in ((0, 0), (8, 1)):
        s1, s2 = float(np.median(p1[off::2])), float(np.median(p2[off::2]))
        out["rects_%d" % k] = dict(stage1_us=s1, stage2_us=s2, us=s1 + s2, ratio_to_digest=(s1 + s2) / out["digest_three_sections"]["us"],
                                   bytes_per_s=20.0 * n / (s1 * 1e-6), min_us=float(min(p1[off::2])) + float(min(p2[off::2])))
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", type=int, default=16_000_000)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--calls", type=int, default=25)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--record-rects", action="store_true", help="the recording carries the eight rectangles too (default: record 0 only)")
    ap.add_argument("--tiles", type=int, default=0, help="the tiled run's pass on K tiles of device 0, next to the single context's")
    ap.add_argument("--trace-run", action="store_true")
    ap.add_argument("--from-trace", metavar="CSV")
    args = ap.parse_args()
    if args.from_trace:
        from_trace(args)
    elif args.tiles:
        tiled(args)
    elif args.trace_run:
        trace_run(args)
    else:
        measure(args)


if __name__ == "__main__":
    main()
