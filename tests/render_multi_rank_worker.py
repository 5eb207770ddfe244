"""One rank of a two-process sphx_multi run that draws its layer (started by tests/test_gpu_render_multi.py through
torch.distributed.run): the halo records travel over torch.distributed / gloo, the scalars through the library's shared segment.
sphx_multi_render_layer makes no communication; the parent merges the two ranks' layers with yasph2d_amd.render_merge.  Writes this
rank's layer, what sphx_multi_render answered, and its owned particles to OUT/rank<r>.npz."""
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

    import render_reference as rr
    import yasph2d_amd as y
    from tiles_reference import cell_coord, quantile_cuts
    from util import dam_break
    from yasph2d_amd.multi import MultiSolver, TorchCommOps

    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    torch.cuda.set_device(0)
    pos, boundary = dam_break(1.0)
    comm = TorchCommOps(dist, torch.device("cuda", 0), shm_name="s" + os.environ.get("MASTER_PORT", "0"))
    m = MultiSolver.rank(y.default_params(), 0, rank, world, comm=comm, halo=10, rebalance_every=4)
    m.set_tiling_invariant(True)
    m.set_strips(0, quantile_cuts(cell_coord(pos, 0), 2))  # two strips along x, cut at the particle-count quantile
    m.set_boundary(boundary)
    m.upload(pos)
    timer = y.TimeManager()
    m.steps(timer, steps)
    view = rr.fit(320, 240, radius=0.015)
    if rank == 1:  # (not collective: one rank alone may draw, and draw twice)
        m.render_layer(**view.fields())
    layer = m.render_layer(**view.fields())
    try:
        m.render(**view.fields())
        code, msg = 0, ""
    except y.SphxError as e:
        code, msg = e.code, str(e)
    d = m.download()
    np.savez(os.path.join(out, f"rank{rank}.npz"), key=layer["key"], owner=layer["owner"], rgba=layer["rgba"], render_code=code, render_msg=msg,
             pos=d["pos"], vel=d["vel"], ids=d["ids"], dt_ns=timer.simulation_step_ns())
    m.close()
    comm.close()
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
