"""One rank of a two-process sphx_multi run that is edited (started by tests/test_gpu_multi_edit.py through torch.distributed.run): the
halo records travel over torch.distributed / gloo, the scalars — and with them the removed counts — through the library's shared segment.
Tiling-invariant mode, fixed 2 + 2 iterations.  Both ranks run the schedule of the tiling-independence test (an emit every 2 steps, a
drain rectangle, a keep-box) with the same arguments, as the collective calls ask, and store what they got."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    out = sys.argv[1]
    import torch
    import torch.distributed as dist

    import yasph2d_amd as y
    from util import dam_break
    from yasph2d_amd import _lib
    from yasph2d_amd.multi import MultiSolver, TorchCommOps

    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    torch.cuda.set_device(0)
    import test_gpu_multi_edit as t  # the schedule itself (module level: constants and helpers only)

    pos, boundary = dam_break(1.0)
    comm = TorchCommOps(dist, torch.device("cuda", 0), shm_name="e" + os.environ.get("MASTER_PORT", "0"))
    m = MultiSolver.rank(y.default_params(**t.INV), 0, rank, world, comm=comm, halo=10, rebalance_every=4)
    m.set_tiling_invariant(True)
    m.set_boundary(boundary)
    m.upload(pos)
    stats, removed, firsts = t.scheduled_run(m)
    d = m.download()
    fields = [k for k, _ in _lib.SphxStepStats._fields_]
    np.savez(os.path.join(out, f"rank{rank}.npz"), removed=np.array(removed, np.uint64), firsts=np.array(firsts, np.uint64),
             stats=np.array([[float(s[k]) for k in fields] for s in stats]), owned=np.array([_lib.lib().sphx_multi_num_owned(m.h)], np.uint64), **d)
    m.close()
    comm.close()
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
