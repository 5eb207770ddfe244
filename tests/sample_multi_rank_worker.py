"""One rank of a two-process sphx_multi run that samples its fields (started by tests/test_gpu_sample_multi.py through
torch.distributed.run): the halo records travel over torch.distributed / gloo, the scalars through the library's shared segment.  The
sampling calls are collective — both ranks call with the same points at the same point of the run — and each returns its own part,
written to OUT/rank<r>.npz; the parent folds the parts with yasph2d_amd.sample_merge."""
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
    from sample_reference import lattice_points
    from util import dam_break
    from yasph2d_amd.multi import MultiSolver, TorchCommOps

    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    torch.cuda.set_device(0)
    pos, boundary = dam_break(1.0)
    F = np.float32
    lattice = (F(-0.07), F(-0.09), F(0.0413), F(0.0391), 57, 71)
    rng = np.random.default_rng(5)  # (the same points on every rank)
    pts = np.concatenate([lattice_points(*lattice)[::2], pos[::7], (pos[::11] + rng.normal(0, 0.02, pos[::11].shape)).astype(F),
                          np.array([[1e6, 1e6], [np.nan, 0.5], [-np.inf, np.inf]], F)]).astype(F)
    comm = TorchCommOps(dist, torch.device("cuda", 0), shm_name="s" + os.environ.get("MASTER_PORT", "0"))
    m = MultiSolver.rank(y.default_params(), 0, rank, world, comm=comm, halo=10, rebalance_every=4)
    m.set_boundary(boundary)
    m.upload(pos)
    m.steps(y.TimeManager(), steps)
    # rank mode without out->tile is refused (the Python wrapper always passes one: the raw call).  The argument check comes before the
    # ghost-band exchange, so the refused call meets no other rank and touches no tile.
    import ctypes as C

    from yasph2d_amd import _lib

    buf = np.zeros(max(len(pts), lattice[4] * lattice[5]), F)  # (large enough for either call, should one not be refused)
    no_tile = _lib.SphxMultiSampleOut(buf.ctypes.data, None, None, None, None)
    before = m.info()["exchanges"]
    refusals = []
    for call in (lambda: m.L.sphx_multi_sample_points(m.h, pts.ctypes.data, len(pts), 0, 0, C.byref(no_tile)),
                 lambda: m.L.sphx_multi_sample_grid(m.h, lattice[0], lattice[1], lattice[2], lattice[3], lattice[4], lattice[5], 0, 0, C.byref(no_tile))):
        rc = call()
        msg = m.L.sphx_multi_last_error(m.h).decode()
        assert rc == _lib.ERR_INVALID_ARGUMENT and "tile" in msg, (rc, msg)
        refusals.append(rc)
    assert m.info()["exchanges"] == before and not buf.any()
    points = m.sample(pts)  # ("tile" comes back in rank mode whether asked for or not)
    grid = m.sample_grid(lattice[:2], lattice[2:4], (lattice[5], lattice[4]))
    save = {"pts": pts, "lattice": np.array(lattice, np.float64), "refused_without_tile": np.array(refusals)}
    for prefix, part in (("points_", points), ("grid_", grid)):
        for k, v in part.items():
            save[prefix + k] = v if v.dtype != np.float32 else v.view(np.uint32)
    np.savez(os.path.join(out, f"rank{rank}.npz"), **save)
    m.close()
    comm.close()
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
