#!/usr/bin/env python3
"""Share of correction workgroups that skip their walk (the zero-correction skip of k_correct) in a window of the
dam-break scene: the scene of bench.py scaled to --particles, --skip-steps untimed steps, then --steps steps over which the counters of
sphx_debug_correction_counts, sphx_debug_quiet_counts, sphx_debug_takeover_counts and sphx_debug_rigid_counts are differenced.  Prints one JSON line.

    python tools/zero_skip_share.py --particles 16000000 --skip-steps 2500 --steps 20
"""
import argparse
import json
import os
import sys

os.environ["SPHX_ZERO_SKIP_COUNT"] = "1"  # read once, in sphx_create
os.environ.setdefault("SPHX_ZERO_SKIP", "1")  # (by default the skip is on from 4 M particles only)
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

import yasph2d_amd as y  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", type=int, default=16_000_000)
    ap.add_argument("--skip-steps", type=int, default=0)
    ap.add_argument("--steps", type=int, default=20)
    args = ap.parse_args()
    w = y.FluidParticleWorld()
    w.reset_fluid(float(np.sqrt(args.particles / 4050.0)))
    timer = y.TimeManager()
    solver = y.DFSPHSolver(w, y.default_params())
    done = 0
    while done < args.skip_steps:  # (in pieces: one library call per 250 steps)
        k = min(250, args.skip_steps - done)
        solver.simulation_steps(w, timer, k, sync_world=False)
        done += k
    ctx = solver.context()
    c0 = np.array(ctx.correction_counts(), np.int64)
    q0 = np.array(ctx.quiet_counts(), np.int64)
    t0 = np.array(ctx.takeover_counts(), np.int64)
    r0 = np.array(ctx.rigid_counts(), np.int64)
    stats = solver.simulation_steps(w, timer, args.steps, sync_world=False)
    c1 = np.array(ctx.correction_counts(), np.int64)
    d = c1 - c0
    q = np.array(ctx.quiet_counts(), np.int64) - q0  # (quiet-scene exits, corrections queued in the decide-first form)
    t = np.array(ctx.takeover_counts(), np.int64) - t0  # (thin launches, producers that stored the warm-start sums, recount moves)
    r = np.array(ctx.rigid_counts(), np.int64) - r0  # (non-pressure passes queued in the rigid form, their rigid exits, their marked runs)
    total = int(d.sum())
    print(json.dumps({
        "particles": len(w.positions), "skip_steps": args.skip_steps, "steps": args.steps,
        "mean_density_iterations": float(np.mean([s["density_iterations"] for s in stats])),
        "mean_divergence_iterations": float(np.mean([s["divergence_iterations"] for s in stats])),
        "correction_workgroups": total, "skipped": int(d[0]), "stopped_by_window_flag": int(d[1]), "stopped_by_remote_entry": int(d[2]),
        "skip_share": (float(d[0]) / total) if total else None, "quiet_exits": int(q[0]), "decide_first_launches": int(q[1]),
        "thin_launches": int(t[0]), "takeover_producers": int(t[1]), "recount_moves": int(t[2]),
        "rigid_launches": int(r[0]), "rigid_exits": int(r[1]), "rigid_marked": int(r[2])}))


if __name__ == "__main__":
    main()
