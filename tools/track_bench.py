#!/usr/bin/env python3
"""Cost of following particles by id (sphx_track_*, sphx_download_by_id) next to what they replace.

  tools/track_bench.py [--particles 1000000] [--warmup 50] [--calls 15] [--blocks 6] [--block-steps 20] [--out profiles/track/track_<n>.json]

The dam-break scene is stepped --warmup times through the solver object; on that state:
  * the look-up pass for m = 16, 1 024 and 16 384 tracked ids (a seeded random choice of the ids): device time of the track_lookup launch
    (sphx_profile_*, median of --calls fetches through device pointers) against the model 4 B per particle, as achieved TB/s, and the
    wall time of a host-path sphx_track_fetch (the call with its copies and its synchronisation);
  * the step rate with an every = 1 recording of 1 024 ids on and off: --blocks blocks of --block-steps steps inside
    sphx_solver_simulation_steps, on / off alternating in one process (the order of the first block alternates too: off, on, on, off, ...),
    host clock around a block that ends in a synchronise, profiler off; the median step time of each kind and the loss in percent;
  * sphx_download_by_id of everything against sphx_download + numpy argsort + scatter on the same box (median wall time).
Prints one JSON line and writes it to --out."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import yasph2d_amd as y  # noqa: E402
from yasph2d_amd import _lib  # noqa: E402


def wall_us(ctx, calls, fn):
    ts = []
    for _ in range(calls):
        ctx.synchronize()
        t0 = time.perf_counter()
        fn()
        ctx.synchronize()
        ts.append((time.perf_counter() - t0) * 1e6)
    return float(np.median(ts))


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", type=int, default=1_000_000)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--calls", type=int, default=15)
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--block-steps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    w = y.FluidParticleWorld()
    w.reset_fluid(float(np.sqrt(args.particles / 4050.0)))
    solver, timer = y.DFSPHSolver(w, y.default_params()), y.TimeManager()
    solver.simulation_steps(w, timer, args.warmup, sync_world=False)
    ctx = solver.context()
    n = ctx.n
    out = dict(particles=n, warmup=args.warmup, calls=args.calls, model_bytes_lookup=4.0 * n)
    rng = np.random.default_rng(1)

    # ---- the look-up pass
    ctx.profile_filter(None)
    ctx.profile_enable(True)
    out["event_overhead_us"] = ctx.profile_event_overhead() * 1e3
    for m in (16, 1024, 16384):
        ids = rng.choice(n, m, replace=False).astype(np.uint32)
        ctx.track(ids)
        dev_out = {"slot": torch.zeros(m, dtype=torch.int32, device="cuda"), "pos": torch.zeros((m, 2), device="cuda"),
                   "vel": torch.zeros((m, 2), device="cuda"), "density": torch.zeros(m, device="cuda")}
        ctx.track_fetch(out=dev_out)  # (warm: code objects)
        lookup, emit = [], []
        for _ in range(args.calls):
            ctx.profile_reset()
            ctx.track_fetch(out=dev_out)
            prof = ctx.profile_get()
            lookup.append(prof["track_lookup"]["total_ms"] * 1e3)
            emit.append(prof["track_emit"]["total_ms"] * 1e3)
        found = int((dev_out["slot"] != -1).sum().item())
        assert found == m
        lu = float(np.median(lookup))
        ctx.profile_enable(False)
        host = wall_us(ctx, args.calls, ctx.track_fetch)
        ctx.profile_enable(True)
        out["lookup_m%d" % m] = dict(lookup_us=lu, lookup_min_us=float(np.min(lookup)), emit_us=float(np.median(emit)),
                                     achieved_TB_per_s=4.0 * n / (lu * 1e-6) / 1e12, fetch_host_wall_us=host)
    ctx.profile_enable(False)

    # ---- the recorder inside the step loop: on / off alternating
    ids = rng.choice(n, 1024, replace=False).astype(np.uint32)
    ctx.track(ids)
    k = args.block_steps
    solver.simulation_steps(w, timer, k, sync_world=False)  # (settle after the fetches)
    ms = {False: [], True: []}
    for b in range(args.blocks):
        for on in ((False, True) if b % 2 == 0 else (True, False)):
            ctx.track_record(k if on else 0)
            ctx.synchronize()
            t0 = time.perf_counter()
            solver.simulation_steps(w, timer, k, sync_world=False)
            ctx.synchronize()
            ms[on].append((time.perf_counter() - t0) * 1e3 / k)
            if on:
                assert ctx.track_status()["frames"] == k
    off, on = float(np.median(ms[False])), float(np.median(ms[True]))
    out["recorder"] = dict(m=1024, every=1, blocks=args.blocks, block_steps=k, ms_per_step_off=off, ms_per_step_on=on, off_all=ms[False], on_all=ms[True],
                           steps_per_s_off=1e3 / off, steps_per_s_on=1e3 / on, loss_percent=(on / off - 1.0) * 100.0,
                           model_share_percent=4.0 / 339.0 * 100.0)
    ctx.track_record(0)

    # ---- the id-ordered download against download + argsort + scatter
    def by_argsort():
        d = ctx.download()
        order = np.argsort(d["ids"])
        return d["pos"][order], d["vel"][order], d["density"][order]

    calls = max(3, args.calls // 3)
    a = ctx.download_by_id(0, n)
    b = by_argsort()
    assert a["present"] == n and a["pos"].tobytes() == b[0].tobytes() and a["density"].tobytes() == b[2].tobytes()
    out["download_by_id_all"] = dict(wall_us=wall_us(ctx, calls, lambda: ctx.download_by_id(0, n)))
    out["download_argsort_scatter"] = dict(wall_us=wall_us(ctx, calls, by_argsort))
    out["argsort_over_by_id"] = out["download_argsort_scatter"]["wall_us"] / out["download_by_id_all"]["wall_us"]
    line = json.dumps(out)
    print(line)
    path = args.out or os.path.join(ROOT, "profiles", "track", "track_%d.json" % args.particles)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
