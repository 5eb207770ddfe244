"""One rank of a two-process sphx_multi run that asks for its per-particle flow fields (started by tests/test_gpu_fields_multi.py through
torch.distributed.run): the halo records travel over torch.distributed / gloo, the scalars through the library's shared segment.  The
call is collective — both ranks call at the same point of the run — and each returns the part of its own tile, written to
OUT/rank<r>.npz; the parent concatenates the parts in rank order."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    out, steps = sys.argv[1], int(sys.argv[2])
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
    comm = TorchCommOps(dist, torch.device("cuda", 0), shm_name="s" + os.environ.get("MASTER_PORT", "0"))
    m = MultiSolver.rank(y.default_params(), 0, rank, world, comm=comm, halo=10, rebalance_every=4)
    m.set_boundary(boundary)
    m.upload(pos)
    m.steps(y.TimeManager(), steps)
    part = m.fields()
    after = m.download()
    assert np.array_equal(part["ids"], after["ids"]) and (part["tile"] == rank).all()
    save = {k: (v if v.dtype != np.float32 else v.view(np.uint32)) for k, v in part.items()}
    np.savez(os.path.join(out, f"rank{rank}.npz"), **save)
    m.close()
    comm.close()
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
