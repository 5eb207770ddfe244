#!/usr/bin/env python3
"""Cost of saving, restoring and fingerprinting a context (sphx_state_save / sphx_state_load / sphx_state_digest).

  tools/state_bench.py [--particles 1000000] [--warmup 50] [--calls 7] [--tiles K] [--out profiles/state/state_<n>.json]

The dam-break scene is stepped --warmup times; on that state, --calls times each (median wall time of the call in ms; every call ends
with the library's own synchronisation):
  * digest                      the nine section digests of the live state (one streaming read of the state, 72 bytes back)
  * save_host / load_host       the blob in host memory (numpy)
  * save_device / load_device   the blob in device memory (SPHX_STATE_DEVICE_BUFFER, a torch tensor)
  * d2d_copy                    a plain device-to-device copy of a tensor of the blob's size (what a copy alone costs)
  * download_upload             the round trip the blob replaces for the arrays it can carry: sphx_download + sphx_download_solver_state,
                                then sphx_upload (which drops what the blob keeps: warm-start arrays, counts, lists)
Loads go into the saving context itself (a rollback: the boundary is kept, one neighbour build runs).  Also reported: the blob's size,
the bytes per particle, and the achieved bandwidth of digest (bytes of the state / time) and of the device save (2 x bytes: one read for
the digests, one copy).  Prints one JSON line and writes it to --out.

--tiles K adds the checkpoint of a tiled run (sphx_multi_state_*) on K in-process tiles of device 0, after the same warm-up: per tile the
local and owned counts and the three launches of the pack pass from the library's hipEvent brackets (mstate_count, mstate_scan,
mstate_pack: median microseconds), the pack's bandwidth against its 36 + 36 * (owned share) bytes per local particle, and the wall time
of the whole calls (multi_digest_ms, multi_save_ms, multi_load_ms) next to the single context's numbers above as the yardstick."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import yasph2d_amd as y  # noqa: E402


def median_ms(calls, fn, sync):
    out = []
    for _ in range(calls):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out))


def bench_tiles(args, world):
    """sphx_multi_state_* on args.tiles in-process tiles: the pack pass per tile (hipEvent brackets) and the calls' wall time"""
    from yasph2d_amd.multi import MultiSolver

    m = MultiSolver(y.default_params(), devices=[0] * args.tiles)
    m.set_boundary(world.boundary_particles)
    fresh = y.FluidParticleWorld()
    fresh.reset_fluid(float(np.sqrt(args.particles / 4050.0)))
    m.upload(fresh.positions)
    m.steps(y.TimeManager(), args.warmup)
    out = dict(tiles=args.tiles, per_tile=[])
    out["multi_digest_ms"] = median_ms(args.calls, m.state_digest, m.synchronize)
    out["multi_save_ms"] = median_ms(args.calls, m.save_state, m.synchronize)
    blob = m.save_state()
    out["part_bytes"] = len(blob)
    ctxs = [m.tile_context(k) for k in range(args.tiles)]
    for c in ctxs:
        c.profile_enable(True)
        c.profile_reset()
    for _ in range(args.calls):
        m.state_digest()
    for k, c in enumerate(ctxs):
        prof = c.profile_get()
        d = c.download(pos=False, vel=False, density=False)
        n_local, owned = len(d["ids"]), int((d["ids"] >> 31).sum())
        row = dict(tile=k, n_local=n_local, owned=owned)
        for name in ("mstate_count", "mstate_scan", "mstate_pack"):
            r = prof.get(name)
            row[name + "_us"] = 1e3 * r["total_ms"] / max(r["launches"], 1) if r else None
        if row["mstate_pack_us"]:
            row["pack_TB_per_s"] = (36.0 * n_local + 36.0 * owned) / (row["mstate_pack_us"] * 1e-6) / 1e12
        out["per_tile"].append(row)
        c.profile_enable(False)
    out["multi_load_ms"] = median_ms(max(3, args.calls // 2), lambda: m.load_state(blob), m.synchronize)
    assert m.save_state() == blob, "a load must put back what was saved"
    m.close()
    return out


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", type=int, default=1_000_000)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--tiles", type=int, default=0, help="also measure sphx_multi_state_* on this many in-process tiles of device 0")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    w = y.FluidParticleWorld()
    w.reset_fluid(float(np.sqrt(args.particles / 4050.0)))
    s = y.DFSPHSolver(w, y.default_params())
    s.simulation_steps(w, y.TimeManager(), args.warmup, sync_world=False)
    ctx = s.context()
    ctx.params = y.default_params()  # (the borrowed view carries none: the device of the tensors)
    n, size = ctx.n, ctx.state_size()
    dev = torch.device("cuda", 0)

    def sync():
        ctx.synchronize()
        torch.cuda.synchronize(dev)

    out = dict(particles=n, boundary=ctx.nb, warmup=args.warmup, calls=args.calls, blob_bytes=size, bytes_per_particle=size / max(n, 1))
    out["digest_ms"] = median_ms(args.calls, ctx.state_digest, sync)
    out["save_host_ms"] = median_ms(args.calls, ctx.save_state, sync)
    out["save_device_ms"] = median_ms(args.calls, lambda: ctx.save_state(device=True), sync)
    host_blob, dev_blob = ctx.save_state(), ctx.save_state(device=True)
    before = ctx.state_digest()
    out["load_host_ms"] = median_ms(args.calls, lambda: ctx.load_state(host_blob), sync)
    out["load_device_ms"] = median_ms(args.calls, lambda: ctx.load_state(dev_blob), sync)
    assert ctx.state_digest() == before and ctx.save_state().tobytes() == host_blob.tobytes(), "a load must put back what was saved"
    other = torch.empty_like(dev_blob)
    out["d2d_copy_ms"] = median_ms(args.calls, lambda: other.copy_(dev_blob), sync)

    def round_trip():
        d = ctx.download()
        ctx.download_solver_state()
        ctx.upload(d["pos"], d["vel"])

    out["download_upload_ms"] = median_ms(max(3, args.calls // 2), round_trip, sync)
    out["digest_TB_per_s"] = size / (out["digest_ms"] * 1e-3) / 1e12
    out["save_device_TB_per_s"] = 2.0 * size / (out["save_device_ms"] * 1e-3) / 1e12
    out["save_device_over_d2d_copy"] = out["save_device_ms"] / out["d2d_copy_ms"]
    out["download_upload_over_save_host_plus_load_host"] = out["download_upload_ms"] / (out["save_host_ms"] + out["load_host_ms"])
    if args.tiles:
        out["multi"] = bench_tiles(args, w)
    line = json.dumps(out)
    print(line)
    path = args.out or os.path.join(ROOT, "profiles", "state", "state_%d.json" % args.particles)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
