"""One rank of a two-process sphx_multi run that takes gauges (started by tests/test_gpu_gauge_multi.py through torch.distributed.run):
the halo records travel over torch.distributed / gloo, the scalars through the library's shared segment.  The gauge call is collective —
both ranks call with the same gauges at the same point of the run — and each returns its own parts, one-shot and recorded, written to
OUT/rank<r>.npz; the parent folds the parts with yasph2d_amd.gauge_merge."""
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
    from yasph2d_amd import _lib
    from yasph2d_amd.multi import MultiSolver, TorchCommOps

    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    torch.cuda.set_device(0)
    pos, boundary = dam_break(1.0)
    F = np.float32
    probes = np.array([[0.15, 0.75], [0.3, 0.9], [0.45, 1.2], [0.58, 1.55], [0.62, 0.76], [1.5, 0.7], [0.3, 2.5], [1e6, -1e6]], F)
    gauges = y._gauge_array([[x, 0.6, 0.0, 0.013, 110] for x in (0.15, 0.3, 0.45, 0.58)] +
                            [[0.02, 0.75 + 0.1 * k, 0.0071, 0.0, 120] for k in range(8)] +
                            [[0.75, 1.9, -0.006, -0.011, 110], [-300.0, -300.0, -0.5, -0.5, 9], [0.3, 0.8, 0.1, 0.1, 1]])
    comm = TorchCommOps(dist, torch.device("cuda", 0), shm_name="g" + os.environ.get("MASTER_PORT", "0"))
    m = MultiSolver.rank(y.default_params(), 0, rank, world, comm=comm, halo=10, rebalance_every=4)
    m.set_boundary(boundary)
    m.probe_record(probes, gauges, 8, 3)  # (before the upload)
    m.upload(pos)
    m.steps(y.TimeManager(), steps)
    # rank mode without out_parts is refused (the Python wrapper always passes one: the raw call), before the ghost-band exchange
    rec = np.zeros(len(gauges), y.GAUGE_REC_DTYPE)
    before = m.info()["exchanges"]
    rc = m.L.sphx_multi_gauge_levels(m.h, gauges.ctypes.data, len(gauges), 0, 0, 0.5, 0, rec.ctypes.data, None, None)
    assert rc == _lib.ERR_INVALID_ARGUMENT and "out_parts" in m.L.sphx_multi_last_error(m.h).decode()
    assert m.info()["exchanges"] == before and not rec.view(np.uint8).any()
    none, parts = m.gauges(gauges)  # (the parts come back in rank mode whether asked for or not; a rank alone has no records)
    assert none is None and parts.shape == (1, len(gauges))
    frames = m.probe_frames()
    assert frames["gauges"] is None and len(frames["info"]) == steps // 3
    np.savez(os.path.join(out, f"rank{rank}.npz"), gauges=gauges, parts=parts, refused_without_parts=np.array(rc), frame_parts=frames["parts"],
             frame_points=frames["points"], frame_point_tile=frames["point_tile"])
    m.close()
    comm.close()
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
