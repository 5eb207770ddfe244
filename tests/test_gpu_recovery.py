"""A context that has returned an error code mid-run computes the oracle's result again once the caller has cleared its cached data
and uploaded a scene.  Each case steps the reference scene in lock-step with the oracle first, so that the context is warm (fused
cell counts, warm starts, alternating sweeps), then provokes the error, then runs 24 steps of a known scene against a fresh oracle,
bit for bit.  Where the errors come from:
  * ERR_NEIGHBOR_PANIC inside step_finish: the neighbour build of the step's re-grid finds a capped particle next to a boundary
    particle; the step is abandoned after its density loop, through step_finish's failure path (a fused count of that loop dropped);
  * SPHX_ERR_INVALID_ARGUMENT from step_finish with a NaN dt after step_begin_law has started phase B on the device;
  * ERR_NONFINITE from step_begin's vmax check (an infinite velocity uploaded mid-run).  No scene here produces it deterministically
    inside step_finish.
sphx_upload itself clears the cell histograms, so the recovery does not depend on which call failed."""
import numpy as np
import pytest
from util import assert_same_state, dam_break, step_pair

import yasph2d_amd as y
from oracle.oracle import Oracle
from yasph2d_amd import _lib

pytestmark = pytest.mark.gpu


def warm_context(steps=3):
    pos, boundary = dam_break(1.0)
    ctx, o = y.SphxContext(), Oracle()
    ctx.set_boundary(boundary)
    o.set_boundary(boundary)
    ctx.upload(pos)
    o.set_particles(pos)
    timer = y.TimeManager()
    for s in range(steps):
        step_pair(ctx, o, timer, what=f"warm-up step {s}")
    return ctx, timer


def recover(ctx, steps=24):
    """clear_cached + upload of the reference scene at scale 0.9 (another particle count), then lock-step with a fresh oracle."""
    pos, boundary = dam_break(0.9)
    ctx.clear_cached()
    ctx.set_boundary(boundary)
    ctx.upload(pos)
    o = Oracle()
    o.set_boundary(boundary)
    o.set_particles(pos)
    timer = y.TimeManager()
    for s in range(steps):
        step_pair(ctx, o, timer, what=f"after the error, step {s}")
    assert_same_state(ctx, o, "after the error")


def dense_blob(k=24, spacing=np.float32(0.002)):
    """k x k particles at a fifth of the fluid spacing, far from the reference scene's walls: every list is capped at 64."""
    g = np.stack(np.meshgrid(np.arange(k), np.arange(k)), -1).reshape(-1, 2).astype(np.float32)
    return (np.array([5.0, 5.0], np.float32) + g * spacing).astype(np.float32)


def blob_oracle(boundary):
    o = Oracle()
    o.timer_fixed(1000)
    o.set_boundary(boundary)
    o.set_particles(dense_blob())
    return o


def panic_wall(boundary):
    """Three boundary particles just under the most crowded particle of the blob after its second step (the blob explodes: it is
    five times the rest density).  Put in place between the two steps, they are first used by the second step's re-grid (the
    static grid is rebuilt lazily): the oracle flags the reference's panic (neighborhood_search.rs:373, bit 1) in that step."""
    o = blob_oracle(boundary)
    o.dfsph_step()
    o.dfsph_step()
    assert not (o.neighbor_flags() & 2)
    counts, _, _ = o.neighbors()
    p = o.positions()[int(np.argmax(counts[:, 0]))]
    assert counts[:, 0].max() >= 64
    return (p + np.array([[-0.005, -0.004], [0.0, -0.004], [0.005, -0.004]], np.float32)).astype(np.float32)


def test_recovery_after_neighbor_panic_in_step_finish():
    ctx, _ = warm_context()
    _, boundary = dam_break(1.0)
    wall = panic_wall(boundary)
    ctx.clear_cached()
    ctx.upload(dense_blob())
    o = blob_oracle(boundary)
    timer = y.TimeManager(fixed_ns=1000)
    diam = np.float32(0.01)
    step_pair(ctx, o, timer, what="dense blob, first step")
    assert o.neighbor_flags() == 1
    ctx.set_boundary(wall)
    o.set_boundary(wall)
    vmax = ctx.step_begin(timer.simulation_step(), timer.law(diam))  # (the lists of the first step are still valid: no build here)
    with pytest.raises(y.SphxError) as e:
        ctx.step_finish(y.duration_as_secs_f32(timer.update_simulation_step(diam, vmax)))
    assert e.value.code == _lib.ERR_NEIGHBOR_PANIC
    o.dfsph_step()
    assert o.neighbor_flags() & 2
    recover(ctx)


def test_recovery_after_nonfinite_dt_in_phase_b():
    """step_finish with a NaN dt after step_begin_law has started phase B on the device: an error, the state is gone (a new step
    is refused until the next upload)."""
    ctx, timer = warm_context()
    ctx.step_begin(timer.simulation_step(), timer.law(np.float32(0.01)))
    with pytest.raises(y.SphxError) as e:
        ctx.step_finish(float("nan"))
    assert e.value.code == _lib.ERR_INVALID_ARGUMENT
    with pytest.raises(y.SphxError) as e:
        ctx.step_begin(timer.simulation_step(), timer.law(np.float32(0.01)))
    assert e.value.code == _lib.ERR_NOT_READY
    recover(ctx)


def test_recovery_after_nonfinite_velocity():
    """ERR_NONFINITE: a re-upload mid-run with an infinite velocity (Duration::from_secs_f32 would panic, timemanager.rs:264)."""
    ctx, timer = warm_context()
    pos, boundary = dam_break(1.0)
    vel = np.zeros_like(pos)
    vel[17] = [np.inf, 0.0]
    ctx.upload(pos, vel)
    with pytest.raises(y.SphxError) as e:
        ctx.step_begin(timer.simulation_step(), timer.law(np.float32(0.01)))
    assert e.value.code == _lib.ERR_NONFINITE
    recover(ctx)
