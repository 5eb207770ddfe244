"""One rank of a two-process sphx_multi run that asks neighbour queries (started by tests/test_gpu_query_multi.py through
torch.distributed.run): the halo records travel over torch.distributed / gloo, the scalars through the library's shared segment.  The
queries are NOT collective: half-way through the run rank 1 alone asks, with points of its own, and the run goes on; at the end both
ranks ask with the same points and each writes its own part to OUT/rank<r>.npz; the parent folds the parts with
yasph2d_amd.query_merge and concatenates the select parts."""
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
    from sample_reference import lattice_points
    from util import dam_break
    from yasph2d_amd import _lib
    from yasph2d_amd.multi import MultiSolver, TorchCommOps

    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    torch.cuda.set_device(0)
    pos, boundary = dam_break(1.0)
    F = np.float32
    h = F(0.02)
    lattice = (F(-0.07), F(-0.09), F(0.0413), F(0.0391), 57, 71)
    rng = np.random.default_rng(5)  # (the same points on every rank)
    pts = np.concatenate([lattice_points(*lattice)[::3], pos[::7], (pos[::11] + rng.normal(0, 0.02, pos[::11].shape)).astype(F),
                          np.array([[1e6, 1e6], [np.nan, 0.5], [-np.inf, np.inf]], F)]).astype(F)
    comm = TorchCommOps(dist, torch.device("cuda", 0), shm_name="s" + os.environ.get("MASTER_PORT", "0"))
    m = MultiSolver.rank(y.default_params(), 0, rank, world, comm=comm, halo=10, rebalance_every=4)
    m.set_boundary(boundary)
    m.upload(pos)
    timer = y.TimeManager()
    m.steps(timer, steps // 2)
    alone = -1
    if rank == 1:  # this rank alone, with its own points: nothing is exchanged, nobody is waited for
        before = m.info()["exchanges"]
        alone = m.query(np.ascontiguousarray(pos[rank::5]), h)["count"]
        m.select([(0.0, 0.0, 2.0, 2.0)])
        assert m.info()["exchanges"] == before
    m.steps(timer, steps - steps // 2)
    # rank mode without out->tile is refused (the Python wrapper always passes one: the raw call)
    cnt = np.zeros(1, np.uint64)
    no_tile = _lib.SphxMultiQueryOut(count=cnt.ctypes.data)
    rc = m.L.sphx_multi_query_radius(m.h, pts.ctypes.data, len(pts), float(h), 0, 0, C.byref(no_tile))
    assert rc == _lib.ERR_INVALID_ARGUMENT and "tile" in m.L.sphx_multi_last_error(m.h).decode()
    save = {"pts": pts, "refused_without_tile": np.array([rc]), "alone_count": np.array(alone)}
    before = m.info()["exchanges"]
    for prefix, walls in (("fluid_", False), ("walls_", True)):
        part = m.query(pts, h, boundary=walls)  # ("tile" comes back in rank mode whether asked for or not)
        for k, v in part.items():
            v = np.asarray(v)
            save[prefix + k] = v if v.dtype != np.float32 else v.view(np.uint32)
    sel = m.select([(0.2, 0.5, 0.9, 1.5)], outside=True)
    for k, v in sel.items():
        save["select_" + k] = np.asarray(v)
    assert m.info()["exchanges"] == before
    for k, v in m.state_digest().items():  # (collective: both ranks)
        save["digest_" + k] = np.array(v, np.uint64)
    np.savez(os.path.join(out, f"rank{rank}.npz"), **save)
    m.close()
    comm.close()
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
