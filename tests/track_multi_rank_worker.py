"""One rank of a two-process sphx_multi run that follows particles by id (started by tests/test_gpu_track_multi.py through
torch.distributed.run): the halo records travel over torch.distributed / gloo, the scalars through the library's shared segment.  The
tracking calls are LOCAL: each rank writes its own part — fetch, by-id download, recorded frames — to OUT/rank<r>.npz, and the parent
folds the parts with yasph2d_amd.track_merge / track_merge_frames."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    out, steps, every = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
    import torch
    import torch.distributed as dist

    import yasph2d_amd as y
    from util import dam_break
    from yasph2d_amd.multi import MultiSolver, TorchCommOps

    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    torch.cuda.set_device(0)
    pos, boundary = dam_break(1.0)
    n = len(pos)
    ids = np.concatenate([np.random.default_rng(5).integers(0, n, 300), [7, 7, n + 3, 2**31 + 1]]).astype(np.uint32)  # (the same on every rank)
    comm = TorchCommOps(dist, torch.device("cuda", 0), shm_name="t" + os.environ.get("MASTER_PORT", "0"))
    m = MultiSolver.rank(y.default_params(), 0, rank, world, comm=comm, halo=10, rebalance_every=4)
    m.set_boundary(boundary)
    m.upload(pos)
    m.track(ids)
    m.track_record(16, every=every)
    timer = y.TimeManager()
    m.steps(timer, steps)
    fetch = m.track_fetch()
    by_id = m.download_by_id(0, n + 5)
    frames, tiles = m.track_frames(tiles=True)
    st = m.track_status()
    save = {"ids": ids, "frames": frames.view(np.uint32), "frame_tiles": tiles, "present": np.array([by_id.pop("present")]),
            "status": np.array([st[k] for k in ("m", "recording", "max_frames", "every", "frames", "dropped")])}
    for k, v in fetch.items():
        save["fetch_" + k] = v.view(np.uint32)
    for k, v in by_id.items():
        save["byid_" + k] = v.view(np.uint32)
    np.savez(os.path.join(out, f"rank{rank}.npz"), **save)
    m.close()
    comm.close()
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
