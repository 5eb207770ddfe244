"""Per-particle flow fields of a tiled run on the device (include/sphx.h, "per-particle flow fields of a tiled run"):
sphx_multi_particle_fields.  The expected values never come from the call under test: they are the float32 restatement of the contract
(tests/fields_reference.py::fields32) over the answering tile's own downloads — arrays, neighbour lists and clipped boundary, ghosts
included — or the single context in tiling-invariant mode, matched by id.  Everything is compared as bits.  All scenes are the dam
break of tests/util.py at scale 1.0 (4 050 particles, every tile on device 0) with small halos and a re-partition every 4 steps, so
that ghosts, migration and moving cuts really happen.  The argument rule behind the single-context equality is checked without a GPU
in tests/test_fields_multi_host.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import fields_reference as fr
import multi_state_reference as mref
import yasph2d_amd as y
from util import dam_break
from yasph2d_amd import _lib
from yasph2d_amd.multi import MultiSolver

pytestmark = pytest.mark.gpu

F = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
POS, BOUNDARY = dam_break(1.0)
N = len(POS)
DIAM = F(0.01)
NAMES = fr.NAMES
SHAPE = dict(vel_grad=(2, 2), divergence=(), vorticity=(), color_grad=(2,))
STEP_FIELDS = tuple(k for k, _ in _lib.SphxStepStats._fields_)
# the fluid lies in the cell columns 5005 .. 5029 at t = 0: the last of these three strips (x >= 1.2, more than a halo away) holds the
# right-hand walls and no fluid, not even a ghost
THREE_STRIPS = (0, [0, 5017, 5060, 65536])
TILINGS = [(1, None), (2, None), (4, None), (3, THREE_STRIPS)]
TILING_IDS = ["one tile", "2 strips", "2x2", "3 strips, one without fluid"]
SUBSET = ("divergence", "color_grad")


def bits(a):
    a = np.ascontiguousarray(a)
    return a if a.dtype == np.uint32 else a.view(np.uint32)


def refused(code, fn, *args, **kw):
    with pytest.raises(y.SphxError) as e:
        fn(*args, **kw)
    assert e.value.code == code, str(e.value)
    return str(e.value)


def new_multi(world, strips=None, params=None, halo=10, rebalance_every=4, invariant=False, **kw):
    m = MultiSolver(params if params is not None else y.default_params(), devices=[0] * world, halo=halo, rebalance_every=rebalance_every, **kw)
    if invariant:
        m.set_tiling_invariant(True)
    if strips is not None:
        m.set_strips(*strips)
    m.set_boundary(BOUNDARY)
    return m


def tile_states(m):
    """every local tile's own arrays, ghosts included, its neighbour lists and its clipped boundary: what the answering tile computes from"""
    out = []
    for k in range(m.info()["local_tiles"]):
        t = m.tile_context(k)
        d = t.download()
        if len(d["ids"]):
            counts, _, lists = t.download_neighbors()
        else:
            counts, lists = np.zeros((0, 2), np.uint16), np.zeros(0, np.uint32)
        out.append(dict(pos=d["pos"], vel=d["vel"], density=d["density"], boundary=t.download_boundary()[0], ids=d["ids"], counts=counts, lists=lists))
    return out


def consts_of(m, params=None):
    return fr.Constants(params if params is not None else m.params, m.tile_context(0).constants())


def reference(K, states):
    """fields32 over every tile's own arrays (ghosts walked like everybody else and then dropped), the owned entries in the tile's
    device order, tile after tile -> dict of the four outputs plus ids and tile"""
    parts = {f: [] for f in NAMES + ("ids", "tile")}
    for t, st in enumerate(states):
        own = (st["ids"] >> 31) == 1
        r = fr.fields32(K, st, st["counts"], st["lists"])
        for f in NAMES:
            parts[f].append(r[f][own])
        parts["ids"].append(st["ids"][own] & np.uint32(0x7FFFFFFF))
        parts["tile"].append(np.full(int(own.sum()), t, np.int32))
    return {f: np.concatenate(v) for f, v in parts.items()}


def assert_bits(dev, ref, what):
    for f in dev:
        a, b = bits(dev[f]), bits(ref[f])
        assert a.shape == b.shape, (what, f, a.shape, b.shape)
        bad = a != b
        assert not bad.any(), "%s: %s differs in %d of %d words, first at %s" % (what, f, int(bad.sum()), bad.size, np.argwhere(bad)[0].tolist())


def pieces(ids):
    """(ghost-only, mixed, fully owned) 256-slot pieces of a tile's id words, and the ghost-only wavefronts inside mixed pieces"""
    own = (np.asarray(ids, np.uint32) >> 31) == 1
    pad = np.zeros((-len(own)) % 256, bool)
    live = np.concatenate([np.ones(len(own), bool), pad]).reshape(-1, 256)
    o = np.concatenate([own, pad]).reshape(-1, 256)
    k, n = o.sum(1), live.sum(1)
    mixed = (k > 0) & (k < n)
    w = o.reshape(-1, 4, 64).sum(2)
    lw = live.reshape(-1, 4, 64).sum(2)
    ghost_waves = int(((w == 0) & (lw > 0))[mixed].sum())
    return int((k == 0).sum()), int(mixed.sum()), int(((k == n) & (n > 0)).sum()), ghost_waves


def snapshot(m, what):
    """everything the device says about one state, taken while the multi is in it"""
    s = dict(what=what, states=tile_states(m))
    s["full"] = m.fields()
    s["after"] = m.download()
    s["alone"] = {f: m.fields(f) for f in NAMES}
    s["subset"] = m.fields(SUBSET)
    return s


@pytest.fixture(scope="module", params=TILINGS, ids=TILING_IDS)
def run40(request):
    """default mode, after the upload and after 40 adaptive steps with a re-partition every 4: (world, multi, constants, snapshots)"""
    world, strips = request.param
    m = new_multi(world, strips)
    m.upload(POS)
    snaps = [snapshot(m, "after the upload")]
    m.steps(y.TimeManager(), 40)
    snaps.append(snapshot(m, "after 40 steps"))
    if world > 1:
        assert m.info()["rebalances"] >= 1, m.info()
    yield world, m, consts_of(m), snaps
    m.close()


# ---- 1. against the answering tile -----------------------------------------------------------------------------------------------------------
def test_bit_identical_to_the_answering_tiles_own_arrays(run40):
    world, m, K, snaps = run40
    for s in snaps:
        what = "%d tiles, %s" % (world, s["what"])
        assert len(s["states"]) == world
        ref = reference(K, s["states"])
        full = s["full"]
        assert tuple(full) == NAMES + ("ids", "tile")
        assert all(full[f].shape == (len(ref["ids"]),) + SHAPE[f] and full[f].dtype == F for f in NAMES)
        assert full["ids"].dtype == np.uint32 and np.array_equal(full["ids"], ref["ids"]), what + ": ids"
        assert full["tile"].dtype == np.int32 and np.array_equal(full["tile"], ref["tile"]), what + ": tile"
        assert_bits({f: full[f] for f in NAMES}, ref, what)
        for f in NAMES:
            got = s["alone"][f]
            assert tuple(got) == (f, "ids", "tile") and np.array_equal(got["ids"], ref["ids"]) and np.array_equal(got["tile"], ref["tile"])
            assert_bits({f: got[f]}, ref, "%s, %s alone" % (what, f))
        assert tuple(s["subset"]) == SUBSET + ("ids", "tile")
        assert_bits(s["subset"], ref, "%s, subset %s" % (what, SUBSET))
        if world > 1:
            assert len(np.unique(full["tile"])) == min(world, 2 if world == 3 else world), what
        # the answer is not trivially zero: the column has a free surface (its velocity gradient may well be: 40 steps in, the column
        # still falls as one body)
        assert np.abs(full["color_grad"]).max() > 1.0
    if world == 2:  # the float64 bound of the restatement, over each tile's own arrays (one tiling)
        for t, st in enumerate(snaps[-1]["states"]):
            own = (st["ids"] >> 31) == 1
            r64, mag, k = fr.fields64(m.params, st, st["counts"], st["lists"])
            dev = {f: snaps[-1]["full"][f][snaps[-1]["full"]["tile"] == t] for f in NAMES}
            r = fr.assert_within_bound(dev, {f: r64[f][own] for f in NAMES}, {f: mag[f][own] for f in NAMES}, k[own], "tile %d after 40 steps" % t)
            print("tile %d: bound ratios %s" % (t, r))


# ---- 2. every particle once ----------------------------------------------------------------------------------------------------------------
def test_every_particle_is_answered_exactly_once(run40):
    world, m, K, snaps = run40
    for s in snaps:
        full, after = s["full"], s["after"]
        assert len(full["ids"]) == N and np.array_equal(np.sort(full["ids"]), np.arange(N, dtype=np.uint32)), s["what"]
        # entry k lines up with entry k of a download made after the call
        assert np.array_equal(full["ids"], after["ids"]), s["what"]
        own = np.concatenate([(st["ids"] >> 31) == 1 for st in s["states"]])
        for f in ("pos", "vel", "density"):
            assert np.array_equal(bits(after[f]), bits(np.concatenate([st[f] for st in s["states"]])[own])), (s["what"], f)
    by_id = m.fields(by_id=True)
    last = snaps[-1]["full"]
    order = np.argsort(last["ids"], kind="stable")
    assert np.array_equal(by_id["ids"], np.arange(N, dtype=np.uint32))
    for f in last:
        assert np.array_equal(bits(by_id[f]), bits(last[f][order])), f


# ---- 3. ghost-only pieces really occur --------------------------------------------------------------------------------------------------------
def test_ghost_only_pieces_and_wavefronts_occur_and_are_skipped_correctly():
    """strips cut at column 5016 with a fixed halo of 16 cells, right after the upload: each tile's Morton order holds whole 256-slot
    pieces of ghost band (a CPU count over the golden scene gives 3 / 12 / 1 and 1 / 12 / 3 ghost-only / mixed / fully owned pieces)"""
    m = new_multi(2, (0, [0, 5016, 65536]), halo=16, fixed_halo=True, rebalance_every=0)
    # (a rotation plus a shear, so that every component of the velocity gradient has something to sum; the layout follows the positions)
    vel = np.stack([F(-1.7) * (POS[:, 1] - F(1.0)) + F(0.3) * POS[:, 0], F(1.7) * (POS[:, 0] - F(0.3)) + F(0.9) * POS[:, 1] * POS[:, 1]], -1).astype(F)
    m.upload(POS, vel)
    states = tile_states(m)
    for t, st in enumerate(states):
        ghost_only, mixed, owned, ghost_waves = pieces(st["ids"])
        print("tile %d: %d ghost-only, %d mixed, %d fully owned pieces; %d ghost-only wavefronts in mixed pieces" % (t, ghost_only, mixed, owned, ghost_waves))
        assert ghost_only >= 1 and mixed >= 1 and ghost_waves >= 1, (t, ghost_only, mixed, owned, ghost_waves)
    K = consts_of(m)
    ref = reference(K, states)
    got = m.fields()
    assert np.array_equal(got["ids"], ref["ids"]) and np.array_equal(got["tile"], ref["tile"])
    assert_bits({f: got[f] for f in NAMES}, ref, "pieces of ghost band")
    assert (np.abs(got["vel_grad"]).reshape(N, 4).max(0) > 0.1).all() and np.abs(got["vorticity"]).max() > 1.0
    for t, st in enumerate(states):  # ... and with a velocity gradient to speak of, the float64 bound once more
        own = (st["ids"] >> 31) == 1
        r64, mag, k = fr.fields64(m.params, st, st["counts"], st["lists"])
        r = fr.assert_within_bound({f: got[f][got["tile"] == t] for f in NAMES}, {f: r64[f][own] for f in NAMES}, {f: mag[f][own] for f in NAMES}, k[own],
                                   "tile %d, sheared upload" % t)
        print("tile %d: bound ratios %s" % (t, r))
    assert_bits({"color_grad": m.fields("color_grad")["color_grad"]}, ref, "pieces of ghost band, colour only")
    m.close()


# ---- 4. against a single context in tiling-invariant mode ------------------------------------------------------------------------------------
def single_context(steps, params):
    ctx = y.SphxContext(params)
    ctx.set_tiling_invariant(True)
    ctx.set_boundary(BOUNDARY)
    ctx.upload(POS)
    if steps == 0:  # (a single context computes the lists and densities of uploaded positions on request)
        ctx.update_neighborhood()
        ctx.update_densities()
    timer = y.TimeManager()
    for _ in range(steps):
        vmax = ctx.step_begin(timer.simulation_step(), timer.law(DIAM))
        ctx.step_finish(y.duration_as_secs_f32(timer.update_simulation_step(DIAM, vmax)))
    return ctx


def single_by_id(ctx):
    d, f = ctx.download(), ctx.fields()
    order = np.argsort(d["ids"], kind="stable")
    assert np.array_equal(d["ids"][order], np.arange(N, dtype=np.uint32))
    return {k: v[order] for k, v in f.items()}


@pytest.mark.parametrize("tiling", TILINGS, ids=TILING_IDS)
def test_tiling_invariant_mode_equals_the_single_context(tiling):
    """set up as tests/test_gpu_multi.py sets the mode up: fixed 2 + 2 iterations, cell mates ordered by id on both sides"""
    world, strips = tiling
    fixed = (2, 2)
    m = new_multi(world, strips, params=y.default_params(fixed_iterations=fixed), halo=16, invariant=True)
    m.upload(POS)
    timer = y.TimeManager()
    for steps in (0, 40):
        if steps:
            m.steps(timer, steps)
        ctx = single_context(steps, y.default_params(fixed_iterations=fixed))
        got = m.fields(by_id=True)
        assert np.array_equal(got["ids"], np.arange(N, dtype=np.uint32))
        assert_bits({f: got[f] for f in NAMES}, single_by_id(ctx), "%d tiles, %d steps" % (world, steps))
        ctx.close()
    m.close()


# ---- 5. spent band ----------------------------------------------------------------------------------------------------------------------------
def test_a_spent_ghost_band_is_refreshed_by_the_query():
    """fixed halo of 7 cells, 2 density and 3 divergence iterations: from the second step on the divergence loop (a warm start and three
    iterations: 1 + 2 * 3 rings) ends with valid = 0.  The query then makes the exchange the next step_begin owes."""
    fixed = (2, 3)
    m = new_multi(2, None, params=y.default_params(fixed_iterations=fixed), halo=7, fixed_halo=True, invariant=True)
    m.upload(POS)
    timer = y.TimeManager()
    m.steps(timer, 6)
    rings = m.ghost_rings()
    assert rings["valid"] < 1, rings  # the precondition of this test: the band is spent at the query
    ctx = single_context(6, y.default_params(fixed_iterations=fixed))
    want = single_by_id(ctx)
    before = m.info()["exchanges"]
    got = m.fields(by_id=True)
    assert m.info()["exchanges"] == before + 1
    after = m.ghost_rings()
    assert after["valid"] == 7 and after["avalid"] == 6, after
    assert_bits({f: got[f] for f in NAMES}, want, "spent band")
    again = m.fields(by_id=True)
    assert m.info()["exchanges"] == before + 1  # (the second call found a full band)
    assert_bits({f: again[f] for f in NAMES}, want, "spent band, second call")
    m.step_begin(timer.simulation_step())
    assert m.info()["exchanges"] == before + 1  # ... and so does the step: the exchange it owed has happened
    ctx.close()
    m.close()


# ---- 6. no trace in the run -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 4], ids=["2 strips", "2x2"])
def test_calls_leave_no_trace_in_the_run(world):
    runs = []
    for calling in (False, True):
        m = new_multi(world)
        m.upload(POS)
        timer = y.TimeManager()
        stats = []
        for k in range(40):
            stats.append(m.step(timer))
            if calling:
                m.fields(NAMES if k % 2 else ("vorticity",))
        d = m.download()
        order = np.argsort(d["ids"], kind="stable")
        digest = m.state_digest()
        m.step_begin(timer.simulation_step())
        runs.append(dict(stats=stats, d={k: v[order] for k, v in d.items()}, digest=digest, exchanges=m.info()["exchanges"], rebalances=m.info()["rebalances"]))
        m.close()
    a, b = runs
    for k in range(40):
        assert set(STEP_FIELDS) - {"reserved"} <= set(a["stats"][k]) and a["stats"][k] == b["stats"][k], (k, a["stats"][k], b["stats"][k])
    for f in a["d"]:
        assert np.array_equal(bits(a["d"][f]), bits(b["d"][f])), f
    assert a["digest"] == b["digest"] and a["exchanges"] == b["exchanges"] and a["rebalances"] == b["rebalances"] >= 1


# ---- 7. refusals and no-ops ----------------------------------------------------------------------------------------------------------------
def test_refusals_and_no_ops():
    bad, not_ready, capacity = _lib.ERR_INVALID_ARGUMENT, _lib.ERR_NOT_READY, _lib.ERR_CAPACITY
    m = new_multi(2)
    L = m.L
    cap = N + 64
    arr = dict(vel_grad=np.full(4 * cap, np.nan, F), divergence=np.full(cap, np.nan, F), vorticity=np.full(cap, np.nan, F), color_grad=np.full(2 * cap, np.nan, F),
               ids=np.full(cap, 0xFFFFFFFF, np.uint32), tile=np.full(cap, -7, np.int32))
    o = _lib.SphxMultiFieldsOut(*[arr[f].ctypes.data for f in NAMES + ("ids", "tile")])
    untouched = {f: a.copy() for f, a in arr.items()}

    def call(flags=0, out=o, n=cap, n_null=False):
        cnt = C.c_uint64(n)
        rc = L.sphx_multi_particle_fields(m.h, flags, C.byref(out) if out is not None else None, None if n_null else C.byref(cnt))
        return rc, L.sphx_multi_last_error(m.h).decode(), cnt.value

    def nothing_written():
        return all(np.array_equal(bits(arr[f]), bits(untouched[f])) for f in arr)

    # arguments first (they name the argument), before the first upload too
    assert L.sphx_multi_particle_fields(None, 0, C.byref(o), C.byref(C.c_uint64(cap))) == bad
    rc, msg, _ = call(out=None)
    assert rc == bad and "out is NULL" in msg
    rc, msg, _ = call(n_null=True)
    assert rc == bad and "inout_n is NULL" in msg
    rc, msg, _ = call(out=_lib.SphxMultiFieldsOut())
    assert rc == bad and "requests no output" in msg
    rc, msg, _ = call(out=_lib.SphxMultiFieldsOut(None, None, None, None, arr["ids"].ctypes.data, arr["tile"].ctypes.data))  # ids and tile are no fields
    assert rc == bad and "requests no output" in msg
    rc, msg, _ = call(flags=1)
    assert rc == bad and "flags" in msg and "device-pointer" in msg
    # before the first upload
    rc, msg, _ = call()
    assert rc == not_ready and "upload" in msg
    assert nothing_written()
    m.upload(POS)
    exchanges = m.info()["exchanges"]
    # the capacity: the count comes back, nothing is written
    rc, msg, n = call(n=N - 1)
    assert rc == capacity and n == N and "inout_n" in msg
    rc, msg, n = call(n=0)
    assert rc == capacity and n == N
    assert nothing_written() and m.info()["exchanges"] == exchanges
    rc, msg, n = call()
    assert rc == 0 and n == N, msg
    assert not np.isnan(arr["vel_grad"][:4 * N]).any() and np.isnan(arr["vel_grad"][4 * N:]).all() and np.isnan(arr["divergence"][N:]).all()
    assert np.array_equal(np.sort(arr["ids"][:N]), np.arange(N, dtype=np.uint32)) and (arr["ids"][N:] == 0xFFFFFFFF).all()
    assert set(arr["tile"][:N].tolist()) == {0, 1} and (arr["tile"][N:] == -7).all()
    rc, msg, n = call(n=N)  # the exact capacity
    assert rc == 0 and n == N
    # between step_begin and step_finish
    timer = y.TimeManager()
    m.step_begin(timer.simulation_step())
    rc, msg, _ = call()
    assert rc == not_ready and "step" in msg
    m.step_finish(F(0.001))
    assert call()[0] == 0
    # after an edit (it ends in a re-grid)
    removed = m.remove([(-1.0, -1.0, 0.2, 10.0)])
    assert 0 < removed < N
    rc, msg, n = call()
    assert rc == 0 and n == N - removed
    # a multi that a failed state load left broken: one payload word corrupted, the host checks pass, the device digest does not
    blob = m.save_state()
    forged = bytearray(blob)
    forged[mref.parse_part(blob)["table"]["velocities"][0] + 8 * (n // 2)] ^= 0x10
    refused(bad, m.load_state, bytes(forged))
    rc, msg, _ = call()
    assert rc == not_ready and "did not complete" in msg
    m.load_state(blob)  # ... and a load puts it right
    rc, msg, n2 = call()
    assert rc == 0 and n2 == n
    # the plain call still refuses a tile context, and says where to go
    msg = refused(bad, m.tile_context(0).fields)
    assert "tile context" in msg and "sphx_multi_particle_fields" in msg
    # the seam: a plain context is refused, a tile context accepted
    ctx = y.SphxContext()
    got = C.c_uint32()
    fo = _lib.SphxFieldsOut(divergence=arr["divergence"].ctypes.data)
    assert L.sphx_tile_particle_fields_enqueue(ctx.h, _lib.FIELD_BITS["divergence"], 0) == bad and "not a tile context" in L.sphx_last_error(ctx.h).decode()
    assert L.sphx_tile_particle_fields_fetch(ctx.h, C.byref(fo), None, cap, C.byref(got)) == bad and "not a tile context" in L.sphx_last_error(ctx.h).decode()
    assert L.sphx_tile_owned_count(ctx.h, C.byref(got)) == bad
    ctx.close()
    t = m.tile_context(0)
    assert L.sphx_tile_particle_fields_enqueue(t.h, 0, 0) == bad and L.sphx_tile_particle_fields_enqueue(t.h, 16, 0) == bad
    assert L.sphx_tile_particle_fields_fetch(t.h, C.byref(fo), None, cap, C.byref(got)) == not_ready  # nothing queued
    assert L.sphx_tile_particle_fields_enqueue(t.h, _lib.FIELD_BITS["divergence"], 0) == 0
    assert L.sphx_tile_particle_fields_fetch(t.h, C.byref(_lib.SphxFieldsOut(vorticity=arr["vorticity"].ctypes.data)), None, cap, C.byref(got)) == bad  # other fields
    assert L.sphx_tile_particle_fields_fetch(t.h, C.byref(fo), None, 1, C.byref(got)) == capacity and got.value > 1
    m.close()
    # zero owned particles: a successful no-op
    empty = new_multi(2)
    empty.upload(np.zeros((0, 2), F))
    cnt = C.c_uint64(cap)
    keep = {f: a.copy() for f, a in arr.items()}
    assert L.sphx_multi_particle_fields(empty.h, 0, C.byref(o), C.byref(cnt)) == 0 and cnt.value == 0
    assert all(np.array_equal(bits(arr[f]), bits(keep[f])) for f in arr)
    empty.close()


# ---- 8. the solver object --------------------------------------------------------------------------------------------------------------------
def test_solver_object_reaches_the_tiled_fields():
    w = y.FluidParticleWorld()
    w.reset_fluid(1.0)
    s = y.DFSPHMultiSolver(w, [0, 0])
    t = y.TimeManager()
    assert "before the first" in refused(_lib.ERR_NOT_READY, s.fields)  # (the solver uploads with its first step)
    s.simulation_steps(w, t, 5, sync_world=False)
    m = s.multi()
    K = consts_of(m, y.default_params())  # (a borrowed multi carries no params: the solver object runs the defaults)
    ref = reference(K, tile_states(m))
    got = s.fields()
    assert np.array_equal(got["ids"], ref["ids"]) and np.array_equal(got["tile"], ref["tile"]) and len(np.unique(got["tile"])) == 2
    assert_bits({f: got[f] for f in NAMES}, ref, "the solver object's tiles")
    one = s.fields("vorticity", by_id=True)
    assert sorted(one) == ["ids", "tile", "vorticity"] and np.array_equal(one["ids"], np.arange(N, dtype=np.uint32))
    s.close()


# ---- 9. one process per tile ----------------------------------------------------------------------------------------------------------------
def test_rank_mode_parts_concatenate_to_the_in_process_run(tmp_path):
    """Two processes over gloo (the halo records) and the shared segment (the scalars), both on device 0.  Each rank returns its own
    tile's part; the parts in rank order are the bytes of the in-process devices=[0, 0] run, ids in the same order."""
    steps = 12
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1", "--master-port", "29571",
           os.path.join(HERE, "fields_multi_rank_worker.py"), str(tmp_path), str(steps)]
    p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    r = [np.load(tmp_path / f"rank{k}.npz") for k in range(2)]
    m = new_multi(2)
    m.upload(POS)
    m.steps(y.TimeManager(), steps)
    want = m.fields()
    for k in range(2):
        assert len(r[k]["ids"]) > 0 and (r[k]["tile"] == k).all()
    for f in want:
        got = np.concatenate([r[0][f], r[1][f]])
        assert np.array_equal(bits(got), bits(want[f])), f
    m.close()
