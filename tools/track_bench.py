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
Prints one JSON line and writes it to --out.

  tools/track_bench.py --tiles K [--gpus 1] [--particles 1000000] [--warmup 50] [--calls 15] [--blocks 6] [--block-steps 20] [--out profiles/track_multi/...]

The same scene as a tiled run of K tiles (sphx_multi; the tiles are spread over --gpus devices), stepped
--warmup times.  On that state, each new call ALTERNATING with the way a tiled run was followed before it (sphx_multi_download of every
array of every tile, ghosts included, then a host argsort), median host wall time of --calls calls that end synchronised, after one
untimed call of each kind:
  * sphx_multi_track_fetch of m = 16, 1 024 and 16 384 ids against download + argsort + gather of those ids;
  * one recorder frame of 1 024 ids: the step time with an every = 1 recording on and off (blocks alternating as above);
  * sphx_multi_download_by_id of everything against download + argsort + scatter.
Every answer is compared with the old way's before it is timed.  The bytes each way moves over the bus are printed next to the times."""
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


def alternating_us(m, calls, new, old):
    """median wall time (us) of `new` and `old`, one call of each in turn, every call between two synchronisations"""
    new(), old()  # (untimed: code objects, buffers grown on demand)
    ts = {0: [], 1: []}
    for _ in range(calls):
        for k, fn in enumerate((new, old)):
            m.synchronize()
            t0 = time.perf_counter()
            fn()
            m.synchronize()
            ts[k].append((time.perf_counter() - t0) * 1e6)
    return float(np.median(ts[0])), float(np.median(ts[1])), ts[0], ts[1]


def main_tiles(args):
    from yasph2d_amd.multi import MultiSolver

    w = y.FluidParticleWorld()
    w.reset_fluid(float(np.sqrt(args.particles / 4050.0)))
    pos, boundary = np.array(w.positions), np.array(w.boundary_particles)
    gpus = max(1, args.gpus)
    m = MultiSolver(y.default_params(), devices=[k % gpus for k in range(args.tiles)])
    m.set_boundary(boundary)
    m.upload(pos)
    timer = y.TimeManager()
    m.steps(timer, args.warmup)
    m.synchronize()
    n = len(pos)
    n_local = sum(m.tile_context(k).n for k in range(args.tiles))
    out = dict(particles=n, tiles=args.tiles, gpus=gpus, warmup=args.warmup, calls=args.calls, local_particles_with_ghosts=n_local,
               ghost_share=1.0 - n / n_local, bytes_multi_download=32.0 * n_local)
    rng = np.random.default_rng(1)

    def old_rows(ids):
        d = m.download()
        order = np.argsort(d["ids"], kind="stable")
        at = order[np.searchsorted(d["ids"][order], ids)]
        return d["pos"][at], d["vel"][at], d["density"][at]

    # ---- fetch
    for k in (16, 1024, 16384):
        ids = rng.choice(n, k, replace=False).astype(np.uint32)
        m.track(ids)
        a, b = m.track_fetch(), old_rows(ids)
        assert a["pos"].tobytes() == b[0].tobytes() and a["vel"].tobytes() == b[1].tobytes() and a["density"].tobytes() == b[2].tobytes()
        new_us, old_us, new_all, old_all = alternating_us(m, args.calls, m.track_fetch, lambda: old_rows(ids))
        out["fetch_m%d" % k] = dict(fetch_wall_us=new_us, download_argsort_wall_us=old_us, old_over_new=old_us / new_us, fetch_all_us=new_all,
                                    download_argsort_all_us=old_all, bytes_fetch=24.0 * k * args.tiles, bytes_scanned_on_device=4.0 * n_local)

    # ---- one recorder frame: the step with the recording on and off
    ids = rng.choice(n, 1024, replace=False).astype(np.uint32)
    m.track(ids)
    k = args.block_steps
    m.steps(timer, k)
    ms = {False: [], True: []}
    for b in range(args.blocks):
        for on in ((False, True) if b % 2 == 0 else (True, False)):
            m.track_record(k if on else 0)
            m.synchronize()
            t0 = time.perf_counter()
            m.steps(timer, k)
            m.synchronize()
            ms[on].append((time.perf_counter() - t0) * 1e3 / k)
            if on:  # (the last frame is the fetch made now)
                assert m.track_status()["frames"] == k
                frames, tiles = m.track_frames(k - 1, 1, tiles=True)
                f = m.track_fetch()
                assert frames[0, :, :2].tobytes() == f["pos"].tobytes() and np.array_equal(tiles[0], f["tile"])
    off, on = float(np.median(ms[False])), float(np.median(ms[True]))
    m.track_record(0)
    _, old_us, _, _ = alternating_us(m, max(3, args.calls // 3), lambda: None, lambda: old_rows(ids))
    out["recorder"] = dict(m=1024, every=1, blocks=args.blocks, block_steps=k, ms_per_step_off=off, ms_per_step_on=on, off_all=ms[False], on_all=ms[True],
                           frame_us=(on - off) * 1e3, loss_percent=(on / off - 1.0) * 100.0, download_argsort_per_frame_us=old_us,
                           bytes_frame_on_device=20.0 * 1024 * args.tiles, bytes_scanned_on_device=4.0 * n_local)

    # ---- the id-ordered download
    def old_all():
        d = m.download()
        order = np.argsort(d["ids"], kind="stable")
        return d["pos"][order], d["vel"][order], d["density"][order]

    a, b = m.download_by_id(0, n), old_all()
    assert a["present"] == n and a["pos"].tobytes() == b[0].tobytes() and a["vel"].tobytes() == b[1].tobytes() and a["density"].tobytes() == b[2].tobytes()
    calls = max(3, args.calls // 3)
    new_us, old_us, new_all, old_all_us = alternating_us(m, calls, lambda: m.download_by_id(0, n), old_all)
    out["download_by_id_all"] = dict(wall_us=new_us, download_argsort_scatter_wall_us=old_us, old_over_new=old_us / new_us, all_us=new_all,
                                     download_argsort_all_us=old_all_us, bytes_by_id=32.0 * n + 16.0 * args.tiles)
    line = json.dumps(out)
    print(line)
    path = args.out or os.path.join(ROOT, "profiles", "track_multi", "track_%d_tiles%d.json" % (args.particles, args.tiles))
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write(line + "\n")
    m.close()


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", type=int, default=1_000_000)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--calls", type=int, default=15)
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--block-steps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--tiles", type=int, default=0, help="K > 0: measure the tiled calls (sphx_multi_track_*) on K tiles instead")
    ap.add_argument("--gpus", type=int, default=1, help="with --tiles: the devices 0 .. G - 1 the tiles are spread over")
    args = ap.parse_args()
    if args.tiles > 0:
        return main_tiles(args)
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
