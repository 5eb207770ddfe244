#!/usr/bin/env python3
"""Cost of the physical viscosity model: the bench scene (BASELINE configs[2], the 16 M dam break) with each model in a fresh context.

  tools/viscosity_ab.py [--particles 16000000] [--steps 60] [--warmup 30] [--rounds 2] [--mu 0.01]

Rounds alternate the models (xsph, physical, xsph, physical, ...).  Before a context's first step a scratch context keeps the GPU busy
(bench.py's settled-GPU warm-up: an idle gap slows the steps behind it for ~25 steps), then --warmup untimed steps run.  Per round:
ms per step over --steps steps (device loop, no world sync), then a second pass of --steps steps in which every launch of the
non-pressure pass is bracketed by hipEvents (sphx_profile_*): us per k_nonpressure launch.  Prints one JSON line: per model the median
of the rounds, the per-round figures, and the mean density / divergence iteration counts of the timed steps (the models change the flow,
so the solver loops differ: compare ms per step together with them)."""
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

LABEL = "nonpressure_accel_vmax"


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


def one_round(model, args):
    stop = threading.Event()
    th = threading.Thread(target=busy, args=(stop, args.particles), daemon=True)
    th.start()
    time.sleep(0.3)
    w = scene(args.particles)
    params = y.default_params(viscosity=model, fluid_viscosity=args.mu if model == "physical" else None)
    s = y.DFSPHSolver(w, params)
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
    ms = (time.perf_counter() - t0) * 1e3 / args.steps
    ctx.profile_reset()
    ctx.profile_filter(LABEL, 1)
    ctx.profile_enable(True)
    s.simulation_steps(w, t, args.steps, sync_world=False)
    ctx.synchronize()
    ctx.profile_enable(False)
    p = ctx.profile_get()[LABEL]
    assert ctx.viscosity()[0] == model
    s.close()
    return dict(ms_per_step=ms, nonpressure_us=p["total_ms"] * 1e3 / p["launches"], launches=p["launches"],
                density_iterations=float(np.mean([x["density_iterations"] for x in st])),
                divergence_iterations=float(np.mean([x["divergence_iterations"] for x in st])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", type=int, default=16_000_000)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--mu", type=float, default=0.01)
    args = ap.parse_args()
    runs = {"xsph": [], "physical": []}
    for _ in range(args.rounds):
        for model in ("xsph", "physical"):
            runs[model].append(one_round(model, args))
    out = dict(particles=len(scene(args.particles).positions), steps=args.steps, warmup=args.warmup, fluid_viscosity=args.mu)
    for model, rs in runs.items():
        out[model] = {k: float(np.median([r[k] for r in rs])) for k in rs[0]}
        out[model]["rounds"] = rs
    out["nonpressure_ratio"] = out["physical"]["nonpressure_us"] / out["xsph"]["nonpressure_us"]
    out["step_ratio"] = out["physical"]["ms_per_step"] / out["xsph"]["ms_per_step"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
