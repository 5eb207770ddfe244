#!/usr/bin/env python3
"""Cost of the gauges (sphx_gauge_levels) and of the probe recorder (sphx_probe_record) on the dam break.

  tools/gauge_bench.py [--particles 1000000,16000000] [--warmup 40] [--calls 15] [--block 10] [--rounds 4] [--parent-lib PATH]
  tools/gauge_bench.py --tiles K [the same options]      the tiled run: see tiled()

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


def tiled(n, args):
    """--tiles K: the dam break in K tiles on one device (2 x 2 for K == 4, strips otherwise).
    One-shot: 8 columns x 512 samples as ONE sphx_multi_gauge_levels call (wall time, median) next to the path without it —
    multi.sample of the same points (fraction alone) plus gauge_reduce on the host — with the bytes that cross to the host in each.
    Recorder: alternating blocks of --block steps without and with a recording of those columns and 8 probe points at every = 1, on one
    multi; and the same blocks, all without a recording, on a library of the parent commit (--parent-lib) in a child process."""
    y = load(args.lib)
    from yasph2d_amd.multi import MultiSolver

    scale = float(np.sqrt(n / 4050.0))
    w = y.FluidParticleWorld()
    w.reset_fluid(scale)
    m = MultiSolver(y.default_params(), devices=[0] * args.tiles)
    m.set_boundary(w.boundary_particles)
    m.upload(w.positions)
    t = y.TimeManager()
    m.steps(t, args.warmup)
    m.synchronize()
    xs, y_lo, y_hi, dy = columns(scale)
    gauges = [[x, y_lo, 0.0, dy, SAMPLES] for x in xs]
    points = np.stack([xs, np.full(COLUMNS, 1.0 * scale)], -1).astype(np.float32)
    has = hasattr(m, "gauges") and "sphx_multi_gauge_levels" in y._lib.SIGNATURES
    out = dict(particles=n, tiles=args.tiles, columns=COLUMNS, samples=SAMPLES, library=args.lib or "this")

    def block():
        m.synchronize()
        t0 = time.perf_counter()
        m.steps(t, args.block)
        m.synchronize()
        return (time.perf_counter() - t0) * 1e6 / args.block

    if has:
        g = y._gauge_array(gauges)
        k = np.arange(SAMPLES, dtype=np.float32)
        pts = np.concatenate([np.stack([np.full(SAMPLES, np.float32(r["x0"]), np.float32), (np.float32(r["y0"]) + (k * np.float32(r["dy"])).astype(np.float32))], -1)
                              for r in g]).astype(np.float32)
        old = lambda: y.gauge_reduce(m.sample(pts, fields=("fraction",))["fraction"], g, 0.5)
        for _ in range(3):  # warm both ways: code objects, the scratch
            m.gauges(g)
            old()
        call_med, call_min, rec = wall_us(args.calls, lambda: m.gauges(g))
        old_med, old_min, rec_old = wall_us(args.calls, old)
        call_med2, call_min2, _ = wall_us(args.calls, lambda: m.gauges(g))  # (again, behind the other: the spread)
        assert rec.tobytes() == rec_old.tobytes() and (rec["inside"] > 0).all()
        out["one_shot"] = dict(gauge_levels_wall_us=dict(median=call_med, min=call_min, again_median=call_med2, again_min=call_min2),
                               sample_plus_reduce_wall_us=dict(median=old_med, min=old_min), ratio_median=old_med / call_med,
                               bytes_to_host=dict(gauge_levels=32 * COLUMNS * args.tiles, sample_plus_reduce=24 * COLUMNS * SAMPLES),
                               bytes_to_device=dict(gauge_levels=0, sample_plus_reduce=8 * COLUMNS * SAMPLES * args.tiles),
                               levels=[float(v) for v in rec["y"]])
    off, on = [], []
    block()  # (one block unmeasured)
    for _ in range(args.rounds):
        off.append(block())
        if has and not args.no_record:
            m.probe_record(points, gauges, max_frames=args.block, every=1)
        ex0 = m.info()["exchanges"]
        on.append(block())
        ex1 = m.info()["exchanges"]
        if has and not args.no_record:
            assert m.probe_status()["frames"] == args.block
            m.probe_record(max_frames=0)
    out.update(recording=bool(has and not args.no_record), first_blocks_us=off, second_blocks_us=on, step_us_first=float(np.median(off)),
               step_us_second=float(np.median(on)), exchanges_per_step_last_block=(ex1 - ex0) / args.block)
    m.close()
    return out


def tiled_all(n, args):
    """this library with the recording, and — with --parent-lib — the parent's library before and after it, in child processes"""
    def run(lib, no_record):
        cmd = [sys.executable, os.path.abspath(__file__), "--tiles", str(args.tiles), "--tiled-child", str(n), "--warmup", str(args.warmup), "--block",
               str(args.block), "--rounds", str(args.rounds), "--calls", str(args.calls)]
        cmd += (["--lib", lib] if lib else []) + (["--no-record"] if no_record else [])
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=1500)
        if r.returncode != 0:
            raise RuntimeError("child failed: %s\n%s" % (" ".join(cmd), r.stderr[-2000:]))
        return json.loads(r.stdout.strip().splitlines()[-1])

    runs = ([run(args.parent_lib, True)] if args.parent_lib else []) + [run(None, False)] + \
        ([run(args.parent_lib, True), run(None, True)] if args.parent_lib else [])
    return dict(runs=runs)


def main():
    ap = argparse.ArgumentParser()


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
    ap.add_argument("--tiles", type=int, default=0, help="K > 0: the tiled run (sphx_multi_gauge_levels, sphx_multi_probe_record) in K tiles on device 0")
    ap.add_argument("--tiled-child", type=int, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.tiled_child is not None:
        print(json.dumps(tiled(args.tiled_child, args)), flush=True)
        return
    if args.tiles:
        for n in args.particles.split(","):
            print(json.dumps(dict(particles=int(n), tiles=args.tiles, **tiled_all(int(n), args))), flush=True)
        return
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
