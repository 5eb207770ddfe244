"""One rank of a two-process sphx_multi run that is checkpointed (started by tests/test_gpu_multi_state.py through torch.distributed.run):
the halo records travel over torch.distributed / gloo, the scalars — and with them the digests — through the library's shared segment.
Tiling-invariant mode, fixed 2 + 2 iterations.  Each rank runs `before` steps, writes its part to OUT/ckpt.rRRRofWWW, runs `after` more
and stores the result; then every rank loads the complete set of part files again, runs `after` steps once more and stores that too."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    out, before, after = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
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
    comm = TorchCommOps(dist, torch.device("cuda", 0), shm_name="m" + os.environ.get("MASTER_PORT", "0"))
    m = MultiSolver.rank(y.default_params(fixed_iterations=(2, 2)), 0, rank, world, comm=comm, halo=10, rebalance_every=4)
    m.set_tiling_invariant(True)
    m.set_boundary(boundary)
    m.upload(pos)
    timer = y.TimeManager()
    m.steps(timer, before)
    path = os.path.join(out, "ckpt")
    m.save_state_file(path)
    part = m.save_state()
    dig_saved = m.state_digest()  # collective
    tstate = timer.get_state()
    stats_a = m.steps(timer, after)
    d_a = m.download()
    dist.barrier()  # every rank's part file is complete
    m.load_state_file(path)  # collective: every rank reads all parts
    dig_loaded = m.state_digest()
    timer.set_state(tstate)
    stats_b = m.steps(timer, after)
    d_b = m.download()
    fields = [k for k, _ in _lib.SphxStepStats._fields_]
    np.savez(os.path.join(out, f"rank{rank}.npz"), part=np.frombuffer(part, np.uint8),
             dig_saved=np.array([dig_saved[s] for s in _lib.MULTI_STATE_SECTIONS], np.uint64),
             dig_loaded=np.array([dig_loaded[s] for s in _lib.MULTI_STATE_SECTIONS], np.uint64),
             stats_a=np.array([[float(s[k]) for k in fields] for s in stats_a]), stats_b=np.array([[float(s[k]) for k in fields] for s in stats_b]),
             timer=np.frombuffer(bytes(tstate), np.uint8), dt_ns=np.array([timer.simulation_step_ns()], np.uint64),
             **{k + "_a": v for k, v in d_a.items()}, **{k + "_b": v for k, v in d_b.items()})
    m.close()
    comm.close()
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
