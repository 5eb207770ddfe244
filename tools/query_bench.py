#!/usr/bin/env python3
"""Cost of the neighbour queries (sphx_query_radius / sphx_select) on the bench scene (the dam break), next to their yardsticks.

  tools/query_bench.py [--particles 16000000] [--warmup 40] [--calls 15] [--points 1000000]
  tools/query_bench.py --tiles 1,2,4,8 [...]      the tiled calls instead (see run_tiles below)

As tools/sample_bench.py: a scratch context keeps the GPU busy until the context's first step is queued, then --warmup untimed steps
settle the flow.  Measured on that settled state, for --points points uniform in the fluid's bounding box, sorted by cell (Morton order
of cell_of) and in random order, at radius h, through device pointers (torch tensors; nothing crosses to the host):
  * yardstick: sphx_sample_points with only the count output — the same walk in one pass;
  * count:     sphx_query_radius with offsets and nearest, no list (query_count + query_carry + query_offsets);
  * lists:     ... with index, id and dist_sq (query_count + query_carry + query_emit), and the bytes it streams, 12 * total + 8 * m;
  * select:    sphx_select over a rectangle holding about half the fluid (select_flag + select_scan + select_emit), next to the flag and
               scan passes of one sphx_remove over the same rectangle (remove_flag + remove_scan; done last: it edits the state).
Device time per call = the sum of the hipEvent brackets of its launches (sphx_profile_*), median over --calls calls.
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

sys.path.insert(0, os.path.join(ROOT, "tools"))
from sample_bench import busy, part1by1, scene  # noqa: E402


def timed(ctx, labels, calls, fn):
    """median over the calls of the summed device time (us) of the labelled launches, and the per-label medians"""
    tot, per = [], {lab: [] for lab in labels}
    for _ in range(calls):
        ctx.profile_reset()
        fn()
        ctx.synchronize()
        p = ctx.profile_get()
        us = {lab: p[lab]["total_ms"] * 1e3 if lab in p else 0.0 for lab in labels}
        tot.append(sum(us.values()))
        for lab in labels:
            per[lab].append(us[lab])
    return float(np.median(tot)), {lab: float(np.median(v)) for lab, v in per.items()}


TILE_PASSES = ("tile_query_own_flag", "tile_query_own_scan", "tile_query_own_list", "query_count", "query_carry", "query_emit", "query_offsets")
SELECT_PASSES = ("tile_select_flag", "tile_select_scan", "tile_select_emit")


def wall_us(calls, fn):
    ts, res = [], None
    for _ in range(calls):
        t0 = time.perf_counter()
        res = fn()
        ts.append((time.perf_counter() - t0) * 1e6)
    return float(np.median(ts)), res


def sorted_points(pos, m, p):
    """m points uniform in the bounding box of pos, sorted by cell (Morton order of cell_of)"""
    lo, hi = pos.min(0), pos.max(0)
    pts = (lo + np.random.default_rng(1).random((m, 2), dtype=np.float32) * (hi - lo)).astype(np.float32)
    cell = np.fmin(np.fmax((pts - np.array(p.grid_min[:], np.float32)) * np.float32(np.float32(1) / np.float32(p.smoothing_length)), 0), 65535).astype(np.uint32)
    order = np.argsort((part1by1(cell[:, 1]) << np.uint64(1)) | part1by1(cell[:, 0]), kind="stable")
    return np.ascontiguousarray(pts[order])


def merge_alone_us(calls, res, k):
    """sphx_query_merge alone: the answer split back into the K full-form parts the ranks of a multi-process run would hold, and folded.
    The same fold and the same bytes as inside sphx_multi_query_radius; finding who answers a point walks K * m records here, m there."""
    cnt = np.diff(res["offsets"].astype(np.int64))
    which = np.repeat(res["tile"], cnt)
    parts = []
    for t in range(k):
        mine, e = res["tile"] == t, which == t
        off = np.concatenate(([0], np.cumsum(np.where(mine, cnt, 0)))).astype(np.uint64)
        part = dict(offsets=off, tile=np.where(mine, t, -1).astype(np.int32), count=int(off[-1]))
        part.update({f: np.ascontiguousarray(res[f][e]) for f in ("id", "dist_sq", "slot")})
        part.update({f: res[f] for f in ("nearest_id", "nearest_slot", "nearest_dist_sq")})
        parts.append(part)
    us, got = wall_us(calls, lambda: y.query_merge(parts))
    assert got["count"] == res["count"] and np.array_equal(got["id"], res["id"])
    return us


def run_tiles(n, k, args):
    """K tiles on device 0 (--tiles): per pass the device time summed over the tiles (sphx_profile_* of every tile context), the wall time
    of MultiSolver.query (count only; lists), the host fold alone (merge_alone_us), the bytes that cross to the host, MultiSolver.select, and two yardsticks measured in the same process: (i) the single
    context's sphx_query_radius through host pointers on a single-context run of the same scene, (ii) MultiSolver.download() of the
    run, the first thing a user had to do before these calls existed."""
    scale = float(np.sqrt(n / 4050.0))
    w = y.FluidParticleWorld()
    w.reset_fluid(scale)
    s = y.DFSPHMultiSolver(w, [0] * k)
    t = y.TimeManager()
    s.simulation_steps(w, t, args.warmup, sync_world=False)
    m = s.multi()
    tiles = [m.tile_context(i) for i in range(k)]
    p = y.default_params()
    h = np.float32(p.smoothing_length)
    dl_us, whole = wall_us(3, m.download)
    pts = sorted_points(whole["pos"], args.points, p)
    n_run = len(whole["ids"])
    del whole
    total = m.query(pts, h, lists=False, nearest=False)["count"]
    out = dict(particles=n_run, local_records=int(sum(c.n for c in tiles)), tiles=k, points=len(pts), entries=total, warmup=args.warmup, calls=args.calls)

    def device(passes, fn):
        per = [{q: [] for q in passes} for _ in tiles]
        for c in tiles:
            c.profile_filter(None)
            c.profile_enable(True)
        for _ in range(args.calls):
            for c in tiles:
                c.profile_reset()
            fn()
            for i, c in enumerate(tiles):
                c.synchronize()
                prof = c.profile_get()
                for q in passes:
                    per[i][q].append(prof[q]["total_ms"] * 1e3 if q in prof else 0.0)
        for c in tiles:
            c.profile_enable(False)
        med = [{q: float(np.median(v)) for q, v in one.items()} for one in per]
        return {q: sum(one[q] for one in med) for q in passes}, [sum(one.values()) for one in med]

    passes, per_tile = device(TILE_PASSES, lambda: m.query(pts, h, cap=total))
    out.update(passes_us_summed_over_tiles=passes, device_us_per_tile=per_tile, device_us_summed=sum(per_tile))
    count_wall, _ = wall_us(args.calls, lambda: m.query(pts, h, lists=False))
    list_wall, res = wall_us(args.calls, lambda: m.query(pts, h, cap=total, tiles=True))
    merge_us = merge_alone_us(max(3, args.calls // 3), res, k)
    to_host = 12.0 * total + (8.0 + 12.0 + 4.0 + 8.0) * len(pts)  # entries; offsets, nearest triple, point index and local offset per point
    out.update(count_only_wall_us=count_wall, lists_wall_us=list_wall, host_merge_us=merge_us,
               bytes_to_host=to_host, bytes_up=8.0 * len(pts) * k)
    rect = (-1e9, -1e9, float(np.median(pts[:, 0])), 1e9)
    sel_passes, _ = device(SELECT_PASSES, lambda: m.select([rect]))
    sel_wall, sel = wall_us(args.calls, lambda: m.select([rect]))
    out["select"] = dict(selected=sel["count"], passes_us_summed_over_tiles=sel_passes, wall_us=sel_wall)
    out["yardstick_multi_download_wall_us"] = dl_us
    out["yardstick_multi_download_bytes"] = 24.0 * n_run
    s.close()
    # (i) the single context's host path on the same scene
    w1 = y.FluidParticleWorld()
    w1.reset_fluid(scale)
    s1 = y.DFSPHSolver(w1, y.default_params())
    s1.simulation_steps(w1, y.TimeManager(), args.warmup, sync_world=False)
    ctx = s1.context()
    one_wall, one = wall_us(args.calls, lambda: ctx.query(pts, h, cap=total))
    out["yardstick_single_context_host_path"] = dict(wall_us=one_wall, entries=one["count"], lists_over_it=list_wall / one_wall)
    s1.close()
    print(json.dumps(out), flush=True)


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", type=int, default=16_000_000)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--calls", type=int, default=15)
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--tiles", default=None, help="K1,K2,...: measure sphx_multi_query_radius / sphx_multi_select on K tiles (all on device 0) instead")
    args = ap.parse_args()
    if args.tiles:
        for k in args.tiles.split(","):
            run_tiles(args.particles, int(k), args)
        return
    stop = threading.Event()
    th = threading.Thread(target=busy, args=(stop, args.particles), daemon=True)
    th.start()
    time.sleep(0.3)
    w = scene(args.particles)
    s = y.DFSPHSolver(w, y.default_params())
    t = y.TimeManager()
    s.simulation_steps(w, t, 1, sync_world=False)
    stop.set()
    th.join()
    s.simulation_steps(w, t, args.warmup, sync_world=False)
    ctx = s.context()
    ctx.synchronize()
    n = ctx.n
    pos = ctx.download(vel=False, density=False, ids=False)["pos"]
    lo, hi = pos.min(0), pos.max(0)
    m = args.points
    rng = np.random.default_rng(1)
    pts = (lo + rng.random((m, 2), dtype=np.float32) * (hi - lo)).astype(np.float32)
    p = y.default_params()  # (the parameters the solver was created with)
    h = np.float32(p.smoothing_length)
    cell = np.fmin(np.fmax((pts - np.array(p.grid_min[:], np.float32)) * np.float32(np.float32(1) / np.float32(p.smoothing_length)), 0), 65535).astype(np.uint32)
    order = np.argsort((part1by1(cell[:, 1]) << np.uint64(1)) | part1by1(cell[:, 0]), kind="stable")
    out = dict(particles=n, points=m, warmup=args.warmup, calls=args.calls, event_overhead_us=ctx.profile_event_overhead() * 1e3)
    ctx.profile_reset()
    ctx.profile_filter(None)
    ctx.profile_enable(True)
    for name, q in (("sorted_by_cell", np.ascontiguousarray(pts[order])), ("random_order", pts)):
        tq = torch.from_numpy(q).cuda()
        total = ctx.query(tq, h, lists=False, nearest=False)["count"]
        bufs = dict(offsets=torch.empty(m + 1, dtype=torch.int64, device="cuda"), nearest=torch.empty(m, dtype=torch.int32, device="cuda"),
                    nearest_dist_sq=torch.empty(m, dtype=torch.float32, device="cuda"), count=torch.zeros(1, dtype=torch.int64, device="cuda"))
        ent = dict(index=torch.empty(total, dtype=torch.int32, device="cuda"), id=torch.empty(total, dtype=torch.int32, device="cuda"),
                   dist_sq=torch.empty(total, dtype=torch.float32, device="cuda"))
        yard, _ = timed(ctx, ("sample_points",), args.calls, lambda: ctx.sample(tq, fields=("count",)))
        cnt, cnt_per = timed(ctx, ("query_count", "query_carry", "query_offsets"), args.calls, lambda: ctx.query(tq, h, out=dict(bufs)))
        lst, lst_per = timed(ctx, ("query_count", "query_carry", "query_emit"), args.calls, lambda: ctx.query(tq, h, out=dict(bufs, **ent)))
        streamed = 12.0 * total + 8.0 * m
        out[name] = dict(entries=total, yardstick_sample_count_us=yard, count_us=cnt, count_launches_us=cnt_per, count_over_yardstick=cnt / yard,
                         lists_us=lst, lists_launches_us=lst_per, lists_over_two_yardsticks=lst / (2.0 * yard), streamed_bytes=streamed,
                         streamed_GBps_over_the_second_walk=streamed / max(lst_per["query_emit"], 1e-9) * 1e-3)
        del ent
    rect = (float(lo[0]) - 1.0, float(lo[1]) - 1.0, float(np.median(pos[:, 0])), float(hi[1]) + 1.0)  # about half the fluid
    selected = ctx.select([rect], cap=0)["count"]
    sel_out = dict(index=torch.empty(selected, dtype=torch.int32, device="cuda"), id=torch.empty(selected, dtype=torch.int32, device="cuda"))
    sel, sel_per = timed(ctx, ("select_flag", "select_scan", "select_emit"), args.calls, lambda: ctx.select([rect], out=dict(sel_out)))
    ctx.profile_reset()
    removed = ctx.remove([rect])
    ctx.synchronize()
    prof = ctx.profile_get()
    rem = {lab: prof[lab]["total_ms"] * 1e3 for lab in ("remove_flag", "remove_scan", "remove_move") if lab in prof}
    yard = rem.get("remove_flag", 0.0) + rem.get("remove_scan", 0.0)
    out["select"] = dict(rect=rect, selected=selected, us=sel, launches_us=sel_per, removed_by_sphx_remove=removed, remove_launches_us=rem,
                         flag_and_scan_over_removes=(sel_per["select_flag"] + sel_per["select_scan"]) / yard if yard else None,
                         emit_GBps=(8.0 * n + 8.0 * selected) / max(sel_per["select_emit"], 1e-9) * 1e-3)
    ctx.profile_enable(False)
    s.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
