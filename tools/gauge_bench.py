#!/usr/bin/env python3
"""Cost of the gauges (sphx_gauge_levels) and of the probe recorder (sphx_probe_record) on the dam break.

  tools/gauge_bench.py [--particles 1000000,16000000] [--warmup 40] [--calls 15] [--block 10] [--rounds 4] [--parent-lib PATH]

Per particle count:
  (a) one-shot call.  The scene is stepped --warmup times; 8 columns x 512 samples across the free surface of the standing block are
      then measured as ONE sphx_gauge_levels call with host pointers (wall time around the call, which ends in a stream synchronise;
      median over --calls calls) next to the way to the same heights without it, yasph2d_amd.gauge_elevation: eight sphx_sample_grid
      host calls plus the host loop (wall time, median).  The device time of the call's passes (sphx_profile_*: gauge_table,
      gauge_sample, gauge_reduce) is taken in calls of their own, and that of a recorded frame's launches (probe_points, gauge_sample,
      gauge_reduce) behind single steps.  The heights of the two ways are compared.
  (b) recorder overhead.  Child processes (one library each, one at a time) step the same scene: after the warm-up, --rounds times a
      block of --block steps without a recording and a block with the recording of those 8 columns and 8 probe points at every = 1
      (sphx_solver_simulation_steps, wall time around the block, which ends in a synchronise).  The blocks alternate, so the drift of
      the step time along the run cancels.  With --parent-lib PATH (a libsphx.so built from the parent commit) a child on that
      library runs the same blocks, all without a recording, before and after: the parent's step time on the same box in the same
      session, and the block-to-block spread.
Prints one JSON line per particle count."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COLUMNS, SAMPLES = 8, 512
PASSES = ("gauge_table", "gauge_sample", "gauge_reduce")
FRAME_PASSES = ("probe_points", "gauge_sample", "gauge_reduce")


def load(lib_path):
    """yasph2d_amd over the given library; a library of the parent commit lacks the new symbols, which are then left unbound"""
    if lib_path:
        os.environ["SPHX_LIB"] = lib_path
    import yasph2d_amd as y
    from yasph2d_amd import _lib

    if lib_path:
        raw = C.CDLL(lib_path)
        for name in [n for n in _lib.SIGNATURES if not hasattr(raw, n)]:
            del _lib.SIGNATURES[name]
    return y


def scene(y, n, warmup):
    scale = float(np.sqrt(n / 4050.0))
    w = y.FluidParticleWorld()
    w.reset_fluid(scale)
    s = y.DFSPHSolver(w, y.default_params())
    t = y.TimeManager()
    s.simulation_steps(w, t, warmup, sync_world=False)
    ctx = s.context()
    ctx.synchronize()
    return scale, w, s, t, ctx


def columns(scale):
    """8 columns through the block [0.1, 0.6] x [0.7, 1.7] x scale, from 0.6 to 1.9 x scale: across its free surface"""
    xs = np.linspace(0.15, 0.55, COLUMNS) * scale
    y_lo, y_hi = 0.6 * scale, 1.9 * scale
    dy = (y_hi - y_lo) / (SAMPLES - 1)
    return xs, y_lo, y_hi, dy


def wall_us(calls, fn):
    out = []
    for _ in range(calls):
        t0 = time.perf_counter()
        r = fn()
        out.append((time.perf_counter() - t0) * 1e6)
    return float(np.median(out)), float(np.min(out)), r


def one_shot(n, args):
    y = load(None)
    scale, w, s, t, ctx = scene(y, n, args.warmup)
    xs, y_lo, y_hi, dy = columns(scale)
    ny = int(np.floor((y_hi - y_lo) / dy)) + 1
    gauges = [[x, y_lo, 0.0, dy, ny] for x in xs]
    for _ in range(3):  # warm both ways: code objects, the scratch
        ctx.gauges(gauges)
        y.gauge_elevation(ctx, xs, y_lo, y_hi, dy)
    call_med, call_min, rec = wall_us(args.calls, lambda: ctx.gauges(gauges))
    old_med, old_min, elev = wall_us(args.calls, lambda: y.gauge_elevation(ctx, xs, y_lo, y_hi, dy))
    call_med2, call_min2, _ = wall_us(args.calls, lambda: ctx.gauges(gauges))  # (again, behind the other: the spread)
    assert (rec["inside"] > 0).all() and np.allclose(rec["y"], elev, rtol=1e-5, atol=0), (rec["y"], elev)
    ctx.profile_filter(None)
    ctx.profile_enable(True)
    per = {k: [] for k in PASSES}
    for _ in range(args.calls):
        ctx.profile_reset()
        ctx.gauges(gauges)
        p = ctx.profile_get()
        for k in PASSES:
            per[k].append(p[k]["total_ms"] * 1e3 if k in p else 0.0)
    # the launches of a recorded frame (8 probe points + the 8 columns), behind single steps
    points = np.stack([xs, np.full(COLUMNS, 1.0 * scale)], -1).astype(np.float32)
    ctx.probe_record(points, gauges, max_frames=args.calls, every=1)
    frame = {k: [] for k in FRAME_PASSES}
    for _ in range(args.calls):
        ctx.profile_reset()
        s.simulation_step(w, t, sync_world=False)
        ctx.synchronize()
        p = ctx.profile_get()
        for k in FRAME_PASSES:
            frame[k].append(p[k]["total_ms"] * 1e3 if k in p else 0.0)
    assert ctx.probe_status()["frames"] == args.calls
    ctx.probe_record(max_frames=0)
    ctx.profile_enable(False)
    out = dict(particles=ctx.n, columns=COLUMNS, samples=ny, gauge_levels_wall_us=dict(median=call_med, min=call_min, again_median=call_med2, again_min=call_min2),
               gauge_elevation_wall_us=dict(median=old_med, min=old_min), ratio_median=old_med / call_med, ratio_min=old_min / call_min,
               passes_device_us={k: float(np.median(v)) for k, v in per.items()},
               frame_passes_device_us={k: float(np.median(v)) for k, v in frame.items()}, levels=[float(v) for v in rec["y"]])
    s.close()
    return out


def child(args):
    """step-time blocks on one library; prints one JSON line"""
    y = load(args.lib)
    scale, w, s, t, ctx = scene(y, args.child, args.warmup)
    xs, y_lo, y_hi, dy = columns(scale)
    gauges = [[x, y_lo, 0.0, dy, SAMPLES] for x in xs]
    points = np.stack([xs, np.full(COLUMNS, 1.0 * scale)], -1).astype(np.float32)
    can_record = hasattr(ctx, "probe_record") and "sphx_probe_record" in y._lib.SIGNATURES
    off, on = [], []

    def block():
        ctx.synchronize()
        t0 = time.perf_counter()
        s.simulation_steps(w, t, args.block, sync_world=False)
        ctx.synchronize()
        return (time.perf_counter() - t0) * 1e6 / args.block

    block()  # (one block unmeasured: the run-ahead pipeline is in its steady state)
    for _ in range(args.rounds):
        off.append(block())
        if can_record and not args.no_record:
            ctx.probe_record(points, gauges, max_frames=args.block, every=1)
        on.append(block())
        if can_record and not args.no_record:
            assert ctx.probe_status()["frames"] == args.block
            ctx.probe_record(max_frames=0)
    print(json.dumps(dict(particles=ctx.n, recording=bool(can_record and not args.no_record), first_blocks_us=off, second_blocks_us=on)), flush=True)
    s.close()


def run_child(n, args, lib, no_record):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", str(n), "--warmup", str(args.warmup), "--block", str(args.block), "--rounds", str(args.rounds)]
    if lib:
        cmd += ["--lib", lib]
    if no_record:
        cmd += ["--no-record"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=1500)
    if r.returncode != 0:
        raise RuntimeError("child failed: %s\n%s" % (" ".join(cmd), r.stderr[-2000:]))
    return json.loads(r.stdout.strip().splitlines()[-1])


def overhead(n, args):
    runs = []
    if args.parent_lib:
        runs.append(("parent", run_child(n, args, args.parent_lib, True)))
    runs.append(("this", run_child(n, args, None, False)))
    if args.parent_lib:
        runs.append(("parent", run_child(n, args, args.parent_lib, True)))
        runs.append(("this_no_recording", run_child(n, args, None, True)))
    out = dict(block=args.block, rounds=args.rounds, runs=[dict(library=k, **v) for k, v in runs])
    this = dict(runs)["this"]
    off, on = float(np.median(this["first_blocks_us"])), float(np.median(this["second_blocks_us"]))
    out["step_us_without"] = off
    out["step_us_with_recording"] = on
    out["recording_overhead_us"] = on - off
    out["recording_overhead_percent"] = 100.0 * (on - off) / off
    if args.parent_lib:
        par = [v for k, r in runs if k == "parent" for v in r["first_blocks_us"] + r["second_blocks_us"]]
        out["parent_step_us"] = float(np.median(par))
        out["parent_step_spread_percent"] = 100.0 * (max(par) - min(par)) / float(np.median(par))
        out["recording_over_parent_us"] = on - out["parent_step_us"]
        out["recording_over_parent_percent"] = 100.0 * (on - out["parent_step_us"]) / out["parent_step_us"]
        out["no_recording_over_parent_percent"] = 100.0 * (off - out["parent_step_us"]) / out["parent_step_us"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", default="1000000,16000000")
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--calls", type=int, default=15)
    ap.add_argument("--block", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--parent-lib", default=None, help="a libsphx.so built from the parent commit: its step time in the same session")
    ap.add_argument("--skip-overhead", action="store_true")
    ap.add_argument("--child", type=int, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--lib", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--no-record", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child is not None:
        child(args)
        return
    for n in args.particles.split(","):
        out = dict(one_shot=one_shot(int(n), args))
        if not args.skip_overhead:
            out["recorder"] = overhead(int(n), args)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
