"""One rank of a two-process sphx_multi run with fluid statistics (started by tests/test_gpu_stats_multi.py through
torch.distributed.run): the halo records travel over torch.distributed / gloo, the scalars — and with them the statistics records —
through the library's shared segment.  Every call below is collective.  Writes what this rank received, as bytes, and its owned
particles to OUT/rank<r>.npz."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

INF = float("inf")


def raw(a):
    return np.frombuffer(a.tobytes(), np.uint8)


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
    rects = [(-INF, -INF, INF, INF), (0.2, 0.9, 0.5, 1.4), (5.0, 5.0, 6.0, 6.0)]  # everything, a box across the cut, nothing
    comm = TorchCommOps(dist, torch.device("cuda", 0), shm_name="s" + os.environ.get("MASTER_PORT", "0"))
    m = MultiSolver.rank(y.default_params(), 0, rank, world, comm=comm, halo=10, rebalance_every=4)
    m.set_boundary(boundary)
    m.upload(pos)
    whole0, tiles0 = m.stats(rects, per_tile=True)
    m.stats_record(rects, 16, every=every)
    timer = y.TimeManager()
    m.steps(timer, steps)
    whole, tiles = m.stats(rects, per_tile=True)
    frames, info = m.stats_frames()
    st = m.stats_status()
    d = m.download()
    np.savez(os.path.join(out, f"rank{rank}.npz"), rects=np.array(rects, np.float64), whole0=raw(whole0), tiles0=raw(tiles0), whole=raw(whole),
             tiles=raw(tiles), frames=raw(frames), info=raw(info),
             status=np.array([st[k] for k in ("n_rects", "recording", "max_frames", "every", "frames", "dropped")]),
             pos=d["pos"], vel=d["vel"], density=d["density"], ids=d["ids"])
    m.close()
    comm.close()
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
