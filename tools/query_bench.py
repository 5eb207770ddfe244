#!/usr/bin/env python3
"""Cost of the neighbour queries (sphx_query_radius / sphx_select) on the bench scene (the dam break), next to their yardsticks.

  tools/query_bench.py [--particles 16000000] [--warmup 40] [--calls 15] [--points 1000000]

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


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", type=int, default=16_000_000)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--calls", type=int, default=15)
    ap.add_argument("--points", type=int, default=1_000_000)
    args = ap.parse_args()
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
