"""One rank of a two-process sphx_multi run that extracts its free surface (started by tests/test_gpu_contour_multi.py through
torch.distributed.run): the halo records travel over torch.distributed / gloo, the scalars and the windows' borders through the
library's shared segment.  The contour call is collective — both ranks call with the same lattice at the same point of the run — and
each returns its own part, written to OUT/rank<r>.npz; the parent folds the parts with yasph2d_amd.contour_merge."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    out, steps = sys.argv[1], int(sys.argv[2])
    import ctypes as C

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
    pos, boundary = dam_break(1.0)
    F = np.float32
    lattice = (F(-0.07), F(-0.09), F(0.0213), F(0.0191), 97, 113)
    x0, y0, dx, dy, nx, ny = lattice
    comm = TorchCommOps(dist, torch.device("cuda", 0), shm_name="c" + os.environ.get("MASTER_PORT", "0"))
    m = MultiSolver.rank(y.default_params(), 0, rank, world, comm=comm, halo=10, rebalance_every=4)
    m.set_boundary(boundary)
    m.upload(pos)
    m.steps(y.TimeManager(), steps)
    # rank mode without out->cell is refused (the Python wrapper always passes one: the raw call).  The argument check comes before the
    # ghost-band exchange, so the refused call meets no other rank and touches no tile.
    seg, cnt = np.zeros((64, 4), F), np.full(1, 99, np.uint32)
    no_cell = _lib.SphxMultiContourOut(seg.ctypes.data, None, None, cnt.ctypes.data)
    before = m.info()["exchanges"]
    rc = m.L.sphx_multi_surface_contour(m.h, x0, y0, dx, dy, nx, ny, 0, 0, 0.5, 64, 0, C.byref(no_cell))
    msg = m.L.sphx_multi_last_error(m.h).decode()
    assert rc == _lib.ERR_INVALID_ARGUMENT and "cell" in msg, (rc, msg)
    assert m.info()["exchanges"] == before and not seg.any() and cnt[0] == 99
    part = m.contour((x0, y0), (dx, dy), (ny, nx))  # ("tile" comes back in rank mode whether asked for or not)
    assert part["count"] == len(part["cell"]) and (part["tile"] == rank).all()
    # a capacity three short of this rank's count: the first entries of the same order (both ranks call: the call is collective)
    short = m.contour((x0, y0), (dx, dy), (ny, nx), cap=max(part["count"] - 3, 0))
    save = {"lattice": np.array(lattice, np.float64), "refused_without_cell": np.array(rc), "segments": part["segments"].view(np.uint32), "cell": part["cell"],
            "tile": part["tile"], "count": np.array(part["count"]), "short_segments": short["segments"].view(np.uint32), "short_cell": short["cell"],
            "short_tile": short["tile"], "short_count": np.array(short["count"])}
    np.savez(os.path.join(out, f"rank{rank}.npz"), **save)
    m.close()
    comm.close()
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
