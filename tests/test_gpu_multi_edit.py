"""Emitting and draining fluid in a tiled run on the device (include/sphx.h, "emitting and draining fluid in a tiled run"):
sphx_multi_append / sphx_multi_remove and the solver object's append / remove, against the numpy filter of tests/edit_reference.py, the
edited checkpoint part of tests/multi_edit_reference.py and a single context.  All scenes are the dam break of tests/util.py at scale 1.0
(4 050 particles, every tile on device 0).  The exports, the reference's own hand cases and the host rules (routing, id counter) are checked
without a GPU in tests/test_multi_edit_host.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

import edit_reference as eref
import multi_edit_reference as xref
import multi_state_reference as mref
import yasph2d_amd as y
from util import dam_break
from yasph2d_amd import _lib
from yasph2d_amd.multi import MultiSolver

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
POS, BOUNDARY = dam_break(1.0)
N = len(POS)
STEP_FIELDS = tuple(k for k, _ in _lib.SphxStepStats._fields_)  # every sphx_step_stats field
FIVE = ("positions", "velocities", "particle_id", "kappa", "stiffness")
BAD, NOT_READY, CAPACITY = _lib.ERR_INVALID_ARGUMENT, _lib.ERR_NOT_READY, _lib.ERR_CAPACITY
INF = float("inf")
H, GMIN = np.float32(0.02), np.float32(-100.0)  # smoothing length and grid origin of y.default_params()
THREE_STRIPS = (0, [0, 5017, 5100, 65536])  # (the third strip lies to the right of the fluid and owns nothing)


def refused(code, fn, *args, **kw):
    with pytest.raises(y.SphxError) as e:
        fn(*args, **kw)
    assert e.value.code == code, str(e.value)
    return str(e.value)


def new_multi(world, params=None, rebalance_every=4, halo=10, invariant=False, grid=True, strips=None):
    layout = _lib.LAYOUT_AUTO if grid else _lib.LAYOUT_STRIPS
    m = MultiSolver(params if params is not None else y.default_params(), devices=[0] * world, halo=halo, rebalance_every=rebalance_every, layout=layout)
    if invariant:
        m.set_tiling_invariant(True)
    if strips:
        m.set_strips(*strips)
    return m


def make_multi(world, **kw):
    m = new_multi(world, **kw)
    m.set_boundary(BOUNDARY)
    m.upload(POS)
    return m


def by_id(d):
    o = np.argsort(d["ids"], kind="stable")
    return {k: v[o] for k, v in d.items()}


def same_stats(a, b):
    return all(x[k] == y_[k] or (x[k] != x[k] and y_[k] != y_[k]) for x, y_ in zip(a, b) for k in STEP_FIELDS) and len(a) == len(b)


def same_downloads(a, b, keys=("ids", "pos", "vel", "density")):
    a, b = by_id(a), by_id(b)
    for k in keys:
        assert a[k].tobytes() == b[k].tobytes(), k


def crossing(m):
    """world coordinates of the point where the cuts of a 2 x 2 layout meet (the y cut of the left column)"""
    p = mref.parse_part(m.save_state())
    assert p["axis"] == -1 and (p["nx"], p["ny"]) == (2, 2)
    return float(GMIN + np.float32(p["cuts"][1]) * H), float(GMIN + np.float32(p["cuts"][4]) * H)


def block(x, y0, w=0.1, h=0.1):
    """a block of fluid as FluidParticleWorld.add_fluid_rect lays it (no jitter)"""
    fw = y.FluidParticleWorld()
    fw.add_fluid_rect(x, y0, w, h, 0.0)
    return np.array(fw.positions, np.float32)


def filtered(p, gone):
    """the sections of a parsed part without the particles of the mask"""
    keep = ~gone
    return {k: p[k][keep] for k in mref.SECTIONS[:7]}


def five_digests(s, boundary=BOUNDARY):
    d = mref.run_digests(s["particle_id"], s["positions"], s["velocities"], s["density"], s["alpha"], s["kappa"], s["stiffness"], boundary)
    return {k: d[k] for k in FIVE}


def live_five(m):
    d = m.state_digest()
    return {k: d[k] for k in FIVE}


# ---- 1. kept bits and digests ------------------------------------------------------------------------------------------------------------
def test_remove_keeps_the_survivors_bit_for_bit():
    """Default mode, 2 x 2, adaptive steps, a re-partition every 4: after 20 steps a rectangle over the crossing of the cuts goes, then
    everything outside a keep-box."""
    m = make_multi(4)
    timer = y.TimeManager()
    m.steps(timer, 20)
    xc, yc = crossing(m)
    lo, hi = POS.min(0), POS.max(0)
    edits = [((xc - 0.1, yc - 0.1, xc + 0.1, yc + 0.1), False), ((float(lo[0]) + 0.04, float(lo[1]) - 0.3, float(hi[0]) - 0.04, float(hi[1]) - 0.2), True)]
    count = N
    for rects, outside in edits:
        before, p, ex0 = m.download(), mref.parse_part(m.save_state()), m.info()["exchanges"]
        assert p["positions"].tobytes() == before["pos"].tobytes()  # (the part is the download, in the tiles' order)
        gone = eref.removed_mask(before["pos"], rects, outside)
        assert 0 < gone.sum() < count
        removed = m.remove(rects, outside=outside)
        count -= int(gone.sum())
        assert removed == gone.sum() and _lib.lib().sphx_multi_num_owned(m.h) == count and int(m.stats()["count"][0]) == count
        assert m.info()["exchanges"] == ex0 + 1 and m.info()["owned_local"] == count
        after = by_id(m.download())
        want = by_id({k: v[~gone] for k, v in before.items()})
        for k in ("ids", "pos", "vel"):
            assert after[k].tobytes() == want[k].tobytes(), k
        assert live_five(m) == five_digests(filtered(p, gone))
        # no tile holds a record the predicate removes, owned or ghost
        for k in range(4):
            t = m.tile_context(k).download()
            assert not eref.removed_mask(t["pos"], rects, outside).any(), k
    st = m.steps(timer, 4)  # the run goes on
    assert all(s["flags"] == 0 for s in st) and _lib.lib().sphx_multi_num_owned(m.h) == count
    m.close()


# ---- 2. the no-op ----------------------------------------------------------------------------------------------------------------------------
def test_an_edit_that_changes_nothing_leaves_the_run_untouched():
    a, b = make_multi(4), make_multi(4)
    ta, tb = y.TimeManager(), y.TimeManager()
    a.steps(ta, 6), b.steps(tb, 6)
    ex0, dig0 = a.info()["exchanges"], a.state_digest()
    assert a.remove((50.0, 50.0, 51.0, 51.0)) == 0 and a.remove([]) == 0
    assert a.append(np.zeros((0, 2), np.float32)) == N
    assert a.info()["exchanges"] == ex0 and a.state_digest() == dig0
    sa, sb = a.steps(ta, 6), b.steps(tb, 6)
    assert same_stats(sa, sb) and ta.simulation_step_ns() == tb.simulation_step_ns()
    da, db = a.download(), b.download()
    for k in da:
        assert da[k].tobytes() == db[k].tobytes(), k
    assert a.info()["exchanges"] == b.info()["exchanges"]
    a.close(), b.close()


# ---- 3. equivalence to the checkpoint path ---------------------------------------------------------------------------------------------------
INV = dict(fixed_iterations=(2, 2))


def set_saved_layout(m, p):
    if p["axis"] >= 0:
        m.set_strips(p["axis"], p["cuts"])
    else:
        nx, ny = p["nx"], p["ny"]
        m.set_grid(p["cuts"][:nx + 1], np.array(p["cuts"][nx + 1:], np.uint32).reshape(nx, ny + 1))


def test_an_edit_equals_the_edited_checkpoint():
    """Tiling-invariant mode, fixed 2 + 2 iterations (both warm starts fire): run A edits on the device, run B loads the edited part."""
    params = y.default_params(**INV)
    a = make_multi(4, params=params, invariant=True)
    timer = y.TimeManager()
    a.steps(timer, 6)
    blob, tstate = a.save_state(), timer.get_state()
    p = mref.parse_part(blob)
    xc, yc = crossing(a)
    hole = (xc - 0.1, yc - 0.1, xc + 0.1, yc + 0.1)
    new = block(xc - 0.05, yc - 0.05)  # laid across the crossing, inside the hole
    owners = xref.route(new, xref.layout_rects(p), (GMIN, GMIN), H)
    assert sorted(set(owners.tolist())) == [0, 1, 2, 3], "the block must reach all four tiles"
    gone = eref.removed_mask(p["positions"], hole)
    assert a.remove(hole) == gone.sum() > 0
    first = a.append(new)
    assert first == N == xref.counter_after(None, N)
    ids = first + np.arange(len(new), dtype=np.uint32)
    part = xref.edit_part(blob, keep_mask=~gone, appended=(new, None, ids))
    b = new_multi(4, params=params, invariant=True)
    set_saved_layout(b, p)
    b.load_state(part)
    assert a.state_digest() == b.state_digest(), "the eight digests right after the edit"
    assert _lib.lib().sphx_multi_num_owned(a.h) == N - gone.sum() + len(new) == _lib.lib().sphx_multi_num_owned(b.h)
    tb = y.TimeManager()
    tb.set_state(tstate)
    sa, sb = a.steps(timer, 6), b.steps(tb, 6)
    assert all(s["warmstart_density"] == 1 and s["warmstart_divergence"] == 1 for s in sa), "both warm starts must fire"
    assert same_stats(sa, sb) and timer.simulation_step_ns() == tb.simulation_step_ns()
    same_downloads(a.download(), b.download())
    # the counter after a load: 1 + the greatest id of the checkpoint
    assert b.append(np.zeros((0, 2), np.float32)) == int(ids.max()) + 1 == a.append(np.zeros((0, 2), np.float32))
    a.close(), b.close()


# ---- 4. tiling independence --------------------------------------------------------------------------------------------------------------------
DRAIN = (-INF, -INF, INF, 0.75)
KEEP_BOX = (0.0, 0.0, 3.0, 1.6)


def scheduled_run(m, steps=12):
    """an emit every 2 steps (blocks in the air right of the column, across the y cut), a drain rectangle after step 4, a keep-box after
    step 8 -> (stats, [removed, ...], [first_id, ...])"""
    timer = y.TimeManager()
    stats, removed, firsts = [], [], []
    for k in range(steps):
        stats.append(m.step(timer))
        if k % 2 == 1:
            firsts.append(m.append(block(0.7 + 0.12 * (k // 2), 1.15), np.tile(np.float32([0.0, -0.5]), (81, 1))))
        if k == 3:
            removed.append(m.remove(DRAIN))
        if k == 7:
            removed.append(m.remove(KEEP_BOX, outside=True))
    return stats, removed, firsts


@pytest.fixture(scope="module")
def scheduled():
    """the schedule on 2 x 2 tiles, two strips and one tile, in tiling-invariant mode with fixed 2 + 2 iterations"""
    out = {}
    for world in (4, 2, 1):
        m = make_multi(world, params=y.default_params(**INV), invariant=True)
        stats, removed, firsts = scheduled_run(m)
        out[world] = dict(stats=stats, removed=removed, firsts=firsts, d=by_id(m.download()), count=_lib.lib().sphx_multi_num_owned(m.h))
        m.close()
    return out


@pytest.mark.parametrize("world", [2, 1], ids=["2 strips", "one tile"])
def test_edited_run_does_not_depend_on_the_tiling(scheduled, world):
    a, b = scheduled[4], scheduled[world]
    assert a["removed"] == b["removed"] and a["firsts"] == b["firsts"] and a["count"] == b["count"]
    assert all(r > 0 for r in a["removed"]) and a["firsts"] == [N + 81 * k for k in range(6)]
    assert same_stats(a["stats"], b["stats"])
    for k in ("ids", "pos", "vel", "density"):
        assert a["d"][k].tobytes() == b["d"][k].tobytes(), k
    assert a["count"] == N + 6 * 81 - sum(a["removed"]) == len(a["d"]["ids"])


# ---- 5. the single context as anchor ---------------------------------------------------------------------------------------------------------
def single_steps(ctx, timer, k):
    out = []
    for _ in range(k):
        vmax = ctx.step_begin(timer.simulation_step(), timer.law(np.float32(0.01)))
        out.append(ctx.step_finish(y.duration_as_secs_f32(timer.update_simulation_step(np.float32(0.01), vmax))))
    return out


def test_edited_multi_equals_a_single_context_given_the_edited_download():
    """Tiling-invariant mode, fixed 1 + 1 iterations: no warm-start sum is ever read, so a fresh context that is given the edited download in
    id order (a monotone renumbering: the same order inside every cell) computes the same run."""
    params = y.default_params(fixed_iterations=(1, 1))
    hole, new = (0.25, 1.1, 0.45, 1.3), block(0.3, 1.15)
    m = make_multi(4, params=params, invariant=True)
    tm = y.TimeManager()
    m.steps(tm, 6)
    removed, first = m.remove(hole), m.append(new)
    sm = m.steps(tm, 6)
    dm = by_id(m.download())
    m.close()
    ctx = y.SphxContext(params)
    ctx.set_tiling_invariant(True)
    ctx.set_boundary(BOUNDARY)
    ctx.upload(POS)
    ts = y.TimeManager()
    single_steps(ctx, ts, 6)
    d = ctx.download()
    ctx.close()
    pos, vel, ids, gone = eref.remove(d["pos"], d["vel"], d["ids"], hole)
    assert gone == removed > 0
    pos, vel, ids = eref.append(pos, vel, ids, new, None, first)
    o = np.argsort(ids, kind="stable")
    assert np.array_equal(ids[o], dm["ids"])
    ctx2 = y.SphxContext(params)
    ctx2.set_tiling_invariant(True)
    ctx2.set_boundary(BOUNDARY)
    ctx2.upload(pos[o], vel[o])
    t2 = y.TimeManager()
    t2.set_state(ts.get_state())
    s2 = single_steps(ctx2, t2, 6)
    d2 = ctx2.download()
    ctx2.close()
    r = np.argsort(d2["ids"], kind="stable")  # (ids 0 .. n - 1 = the rank of the multi's ids)
    for k in ("pos", "vel", "density"):
        assert d2[k][r].tobytes() == dm[k].tobytes(), k
    assert t2.simulation_step_ns() == tm.simulation_step_ns()
    for k, (a, b) in enumerate(zip(sm, s2)):
        for f in ("density_iterations", "divergence_iterations", "dt", "dt_prev", "vmax") + (("flags",) if k else ()):  # (a fresh upload's first step carries SPHX_FLAG_WARMUP)
            assert a[f] == b[f], (k, f)


# ---- 6. ghosts of new particles ------------------------------------------------------------------------------------------------------------
def test_new_particles_have_their_ghosts_at_once():
    m = make_multi(4, rebalance_every=0)
    timer = y.TimeManager()
    m.steps(timer, 4)
    p = mref.parse_part(m.save_state())
    xc, yc = crossing(m)
    hole = (xc - 0.1, yc - 0.1, xc + 0.1, yc + 0.1)
    new = block(xc - 0.05, yc - 0.05)
    m.remove(hole)
    first = m.append(new)
    halo = m.info()["halo_now"]
    rects = xref.layout_rects(p)
    cx, cy = xref.cell_coord(new[:, 0], GMIN, H), xref.cell_coord(new[:, 1], GMIN, H)
    ids = first + np.arange(len(new), dtype=np.uint32)
    seen_owned = 0
    for k, (x0, x1, y0, y1) in enumerate(rects):
        t = m.tile_context(k).download()
        own = (cx >= x0) & (cx < x1) & (cy >= y0) & (cy < y1)
        band = (cx >= x0 - halo) & (cx < x1 + halo) & (cy >= y0 - halo) & (cy < y1 + halo) & ~own
        have = t["ids"][(t["ids"] & 0x7FFFFFFF) >= first]
        assert sorted(have.tolist()) == sorted((ids[own] | 0x80000000).tolist() + ids[band].tolist()), k
        assert own.any() and band.any()
        seen_owned += int(own.sum())
    assert seen_owned == len(new)
    m.close()


# ---- 7. growth ---------------------------------------------------------------------------------------------------------------------------------
def test_append_beyond_the_reserve_grows_the_tile():
    params = y.default_params(**INV)
    m = make_multi(4, params=params, invariant=True, rebalance_every=0)
    timer = y.TimeManager()
    m.steps(timer, 4)
    info = m.info()
    # the set-up reserved 1.25 x the owned count + 2 max(2, peers) cap_records + 4 096 slots per tile: more than that into ONE tile
    owned = max(len(m.tile_context(k).download()["ids"]) for k in range(4))
    many = int(1.25 * owned + 2 * max(2, info["peers"]) * info["cap_records"] + 4096) + 1000
    p = mref.parse_part(m.save_state())
    g = np.stack(np.meshgrid(np.arange(270), np.arange(many // 270 + 1)), -1).reshape(-1, 2)[:many].astype(np.float32)  # 270 columns: 3 m wide
    new = (np.float32([0.8, 1.45]) + g * np.float32(1.0 / 90.0)).astype(np.float32)  # in the air right of the column, clear of the cuts' bands: one tile
    owners = xref.route(new, xref.layout_rects(p), (GMIN, GMIN), H)
    assert len(set(owners.tolist())) == 1
    before = five_digests({k: p[k] for k in mref.SECTIONS[:7]})
    assert before == live_five(m)
    first = m.append(new)
    assert first == N and _lib.lib().sphx_multi_num_owned(m.h) == N + many
    d = m.download()
    old = d["ids"] < N
    ss = mref.parse_part(m.save_state())
    keep = ss["particle_id"] < N
    assert five_digests({k: ss[k][keep] for k in mref.SECTIONS[:7]}) == before, "the earlier particles' five sections keep their digests"
    assert old.sum() == N and np.array_equal(np.sort(d["ids"][~old]), first + np.arange(many, dtype=np.uint32))
    st = m.steps(timer, 2)
    assert len(st) == 2 and _lib.lib().sphx_multi_num_owned(m.h) == N + many
    m.close()


# ---- 8. empty tiles ----------------------------------------------------------------------------------------------------------------------------
def test_edits_with_empty_tiles():
    m = new_multi(3, rebalance_every=0, strips=THREE_STRIPS)
    m.set_boundary(BOUNDARY)
    m.upload(POS)
    timer = y.TimeManager()
    m.steps(timer, 3)
    x_cut = float(GMIN + np.float32(THREE_STRIPS[1][1]) * H)
    d = m.download()
    strip = (-INF, -INF, x_cut + 0.01, INF)  # (the first strip and half a cell of the second: whatever fp32 does at the cut)
    first_strip = eref.removed_mask(d["pos"], strip)
    assert m.remove(strip) == first_strip.sum() > 0
    t0 = m.tile_context(0).download()["ids"]
    assert not (t0 >> 31).any() and len(t0) > 0, "the first strip owns nothing and still holds ghosts"
    m.steps(timer, 2)
    left = _lib.lib().sphx_multi_num_owned(m.h)
    assert left == N - first_strip.sum()
    assert m.remove([], outside=True) == left and _lib.lib().sphx_multi_num_owned(m.h) == 0
    assert len(m.download()["ids"]) == 0
    new = block(0.3, 1.0)
    assert m.append(new) == N
    assert _lib.lib().sphx_multi_num_owned(m.h) == len(new)
    m.steps(timer, 2)
    d = m.download()
    assert sorted(d["ids"].tolist()) == list(range(N, N + len(new))) and np.isfinite(d["pos"]).all()
    m.close()


# ---- 9. refusals -------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_multi_untouched():
    m = new_multi(2)
    one = np.float32([[0.3, 1.0]])
    assert "before the first" in refused(NOT_READY, m.remove, (0, 0, 1, 1))
    assert "before the first" in refused(NOT_READY, m.append, one)
    m.set_boundary(BOUNDARY)
    m.upload(POS)
    timer = y.TimeManager()
    m.steps(timer, 3)
    dig, ex0 = m.state_digest(), m.info()["exchanges"]
    nan = float("nan")
    refused(BAD, m.remove, [(0, 0, 1, 1)] * 9)
    refused(BAD, m.remove, (0, nan, 1, 1))
    L = _lib.lib()
    assert L.sphx_multi_remove(m.h, None, 1, 0, None) == BAD and L.sphx_multi_remove(m.h, None, 0, 2, None) == BAD
    assert L.sphx_multi_append(m.h, None, None, 1, None) == BAD
    for bad in ([[nan, 1.0]], [[0.3, nan]], [[INF, 1.0]], [[0.3, -INF]]):
        refused(BAD, m.append, np.float32([[0.3, 1.0]] + bad))
    assert m.state_digest() == dig and m.info()["exchanges"] == ex0
    # inside a step (no digest can be taken there: the step is finished and compared with a twin's that was not disturbed)
    twin = make_multi(2)
    twin.steps(y.TimeManager(), 3)
    assert twin.state_digest() == dig
    dt = y.duration_as_secs_f32(timer.simulation_step_ns())
    for mm in (m, twin):
        mm.step_begin(dt)
        if mm is m:
            assert "step_begin" in refused(NOT_READY, m.remove, (0, 0, 1, 1))
            assert "step_begin" in refused(NOT_READY, m.append, one)
        mm.step_finish(dt)
    assert m.state_digest() == twin.state_digest() and m.info()["exchanges"] == twin.info()["exchanges"]
    twin.close()
    # a load that did not complete: a part whose positions were changed behind the digests' back
    m2 = make_multi(2)
    m2.steps(y.TimeManager(), 2)
    blob = bytearray(m2.save_state())
    p = mref.parse_part(bytes(blob))
    blob[p["table"]["positions"][0] + 1] ^= 0x01
    refused(BAD, m2.load_state, bytes(blob))
    assert "did not complete" in refused(NOT_READY, m2.remove, (0, 0, 1, 1))
    assert "did not complete" in refused(NOT_READY, m2.append, one)
    m2.close()
    # ids run out at 2^31: nothing changes
    m3 = new_multi(2)
    m3.set_boundary(BOUNDARY)
    m3.upload(POS, ids=np.arange(N, dtype=np.uint32) + np.uint32((1 << 31) - N - 1))
    dig3 = m3.state_digest()
    assert m3.append(one) == (1 << 31) - 1  # the last id
    dig3b = m3.state_digest()
    assert dig3b != dig3
    refused(CAPACITY, m3.append, one)
    assert m3.state_digest() == dig3b
    m3.close()
    m.close()


# ---- 10. the solver object ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sync", [True, False], ids=["sync_world", "headless"])
def test_solver_object_appends_and_removes(sync):
    w = y.FluidParticleWorld()
    w.reset_fluid(1.0)
    s = y.DFSPHMultiSolver(w, [0, 0])
    timer = y.TimeManager()
    new = block(0.8, 1.2)
    refused(NOT_READY, s.append, w, new)
    s.simulation_steps(w, timer, 3, sync_world=sync)
    hole = (0.25, 1.1, 0.45, 1.3)
    removed = s.remove(w, hole, sync_world=sync)
    assert removed > 0 and w.num_dynamic_particles == N - removed
    first = s.append(w, new, sync_world=sync)
    assert first == N and w.num_dynamic_particles == N - removed + len(new)
    if sync:
        ids = np.array(w.particle_ids)
        assert len(np.unique(ids)) == len(ids) and sorted(ids[ids >= N].tolist()) == list(range(N, N + len(new)))
        assert not eref.removed_mask(np.array(w.positions)[ids < N], hole).any()
    ex0 = s.multi().info()["exchanges"]
    s.simulation_steps(w, timer, 2, sync_world=True)
    # no re-upload in between (it would renumber the particles 0 .. n - 1 and run a fresh decomposition): the ids survive
    ids = np.sort(w.particle_ids)
    assert ids[-1] == N + len(new) - 1 and len(ids) == N - removed + len(new) and len(np.unique(ids)) == len(ids)
    assert s.multi().info()["exchanges"] > ex0
    s.close()


# ---- 11. rank mode -----------------------------------------------------------------------------------------------------------------------------
def test_two_ranks_edit_like_the_in_process_strips(tmp_path, scheduled):
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1", "--master-port", "29561",
           os.path.join(HERE, "multi_edit_rank_worker.py"), str(tmp_path)]
    p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    r = [np.load(tmp_path / f"rank{k}.npz") for k in range(2)]
    for k in ("removed", "firsts", "stats"):
        assert r[0][k].tobytes() == r[1][k].tobytes(), k
    ref = scheduled[2]
    assert r[0]["removed"].tolist() == ref["removed"] and r[0]["firsts"].tolist() == ref["firsts"]
    assert np.array([[float(s[k]) for k in STEP_FIELDS] for s in ref["stats"]]).tobytes() == r[0]["stats"].tobytes()
    ranks = by_id({k: np.concatenate([r[0][k], r[1][k]]) for k in ("ids", "pos", "vel", "density")})
    for k in ("ids", "pos", "vel", "density"):
        assert ranks[k].tobytes() == ref["d"][k].tobytes(), k
    assert int(r[0]["owned"][0]) + int(r[1]["owned"][0]) == ref["count"]
