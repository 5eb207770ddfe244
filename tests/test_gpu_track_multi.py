"""Following particles by id in a tiled run on the device (include/sphx.h, "following particles by id in a tiled run"):
sphx_multi_track_*, sphx_multi_download_by_id and the merge of the ranks' parts.  The expected values never come from the calls under
test: they are what sphx_multi_download returns (a host table id -> record), the tiles' own tile_context(k).download(), or the single
context.  Everything is compared as bits.  All scenes are the dam break of tests/util.py at scale 1.0 (4 050 particles — not a multiple
of 4 — every tile on device 0) with small halos and a re-partition every 4 steps, so that ghosts, migration and moving cuts really
happen.  The host side of the fold is checked without a GPU in tests/test_track_multi_host.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import yasph2d_amd as y
from util import dam_break
from yasph2d_amd import _lib
from yasph2d_amd.multi import MultiSolver

pytestmark = pytest.mark.gpu

F = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
POS, BOUNDARY = dam_break(1.0)
N = len(POS)
A, W = _lib.TRACK_ABSENT, _lib.TRACK_ABSENT_WORD
OWNED = np.uint32(0x80000000)
FLOATS = ("pos", "vel", "density")
STEP_FIELDS = tuple(k for k, _ in _lib.SphxStepStats._fields_)
STATUS0 = dict(m=0, recording=0, max_frames=0, every=0, frames=0, dropped=0)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def refused(code, fn, *args, **kw):
    with pytest.raises(y.SphxError) as e:
        fn(*args, **kw)
    assert e.value.code == code, str(e.value)
    return str(e.value)


def new_multi(world, params=None, rebalance_every=4, halo=10, strips=None, invariant=False):
    m = MultiSolver(params if params is not None else y.default_params(), devices=[0] * world, halo=halo, rebalance_every=rebalance_every)
    if invariant:
        m.set_tiling_invariant(True)
    if strips is not None:
        m.set_strips(*strips)
    m.set_boundary(BOUNDARY)
    return m


def make_multi(world, **kw):
    m = new_multi(world, **kw)
    m.upload(POS)
    return m


def tile_downloads(m):
    return [m.tile_context(k).download() for k in range(m.info()["local_tiles"])]


def ghost_ids(tiles):
    """ids of particles that sit in the ghost band of some tile (bit 31 clear there), from the tiles' own downloads"""
    g = [t["ids"][(t["ids"] >> 31) == 0] for t in tiles]
    return np.unique(np.concatenate(g)) if g else np.zeros(0, np.uint32)


def id_set(tiles, seed=3):
    """a few hundred random ids, duplicates, ids beyond N, ids >= 2^31 and ids that are ghosts in some tile"""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, N, 600).astype(np.uint32)
    g = ghost_ids(tiles)
    extra = np.array([5, 5, 5, base[0], base[1], N, N + 1, 4 * N, 2**31, 2**31 + 5, 2**32 - 1], np.uint32)
    return np.concatenate([base, extra, g[:: max(1, len(g) // 200)]]).astype(np.uint32), len(g)


def expected(d, ids):
    """the records of `ids` from a sphx_multi_download (host table id -> row): {field: bits}, present mask"""
    order = np.argsort(d["ids"], kind="stable")
    sid = d["ids"][order]
    at = np.searchsorted(sid, ids)
    at_c = np.minimum(at, len(sid) - 1)
    present = (at < len(sid)) & (sid[at_c] == ids)
    row = order[at_c]
    out = {}
    for f in FLOATS:
        want = bits(d[f])[row].copy()
        want[~present] = W
        out[f] = want
    return out, present


def check_answer(got, d, tiles, ids, what):
    """one fetch / by-id answer against the multi download and the tiles' downloads"""
    want, present = expected(d, ids)
    for f in FLOATS:
        assert np.array_equal(bits(got[f]), want[f]), (what, f)
    assert np.array_equal(got["tile"] != A, present) and np.array_equal(got["slot"] != A, present), what
    for k in np.nonzero(present)[0]:
        t, s = int(got["tile"][k]), int(got["slot"][k])
        td = tiles[t]
        assert td["ids"][s] == (ids[k] | OWNED), (what, k, "tile/slot must point at the owned record")
        assert bits(td["pos"][s]).tolist() == want["pos"][k].tolist() and bits(td["density"])[s] == want["density"][k]
    return present


@pytest.fixture(scope="module", params=[1, 2, 4], ids=["one tile", "2 strips", "2x2"])
def run40(request):
    """after the upload and after 40 adaptive steps with a re-partition every 4: (world, multi, [(what, download, tile downloads, ids,
    fetch, fetch again, by-id, by-id again)])"""
    world = request.param
    m = make_multi(world)
    states = []

    def snap(what):
        d, tiles = m.download(), tile_downloads(m)
        ids, n_ghost = id_set(tiles)
        m.track(ids)
        states.append(dict(what=what, d=d, tiles=tiles, ids=ids, n_ghost=n_ghost, fetch=m.track_fetch(), fetch2=m.track_fetch(),
                           by_id=m.download_by_id(0, N), by_id2=m.download_by_id(0, N)))

    snap("after the upload")
    m.steps(y.TimeManager(), 40)
    snap("after 40 steps")
    if world > 1:
        assert m.info()["rebalances"] >= 1, m.info()
    yield world, m, states
    m.close()


# ---- 1. fetch ------------------------------------------------------------------------------------------------------------------------------
def test_fetch_against_the_multi_download(run40):
    world, m, states = run40
    for s in states:
        ids = s["ids"]
        assert len(ids) <= _lib.TRACK_MAX_IDS and m.track_status()["m"] == len(states[-1]["ids"])
        present = check_answer(s["fetch"], s["d"], s["tiles"], ids, "%d tiles, %s" % (world, s["what"]))
        assert np.array_equal(present, ids < N)  # (nothing was edited: exactly the ids below N exist)
        assert (s["fetch"]["tile"][present] < world).all()
        if world > 1:
            assert s["n_ghost"] > 0, "the scene must have ghosts"
        # duplicated ids are answered alike
        for a, b in ((600, 601), (601, 602), (0, 603), (1, 604)):
            assert all(bits(s["fetch"][f][a]).tolist() == bits(s["fetch"][f][b]).tolist() for f in s["fetch"])
        # two identical calls return the same bytes
        assert all(s["fetch"][f].tobytes() == s["fetch2"][f].tobytes() for f in s["fetch"])
    if world > 1:
        a, b = states[0]["fetch"]["tile"][:600], states[1]["fetch"]["tile"][:600]
        assert (a != b).any(), "no tracked id changed its tile in 40 steps"


def test_any_subset_of_the_outputs_gives_the_same_bits(run40):
    world, m, states = run40
    s = states[-1]
    for fields in (("pos",), ("tile",), ("slot", "vel"), ("tile", "density"), ("density", "vel", "pos")):
        got = m.track_fetch(fields)
        assert sorted(got) == sorted(fields)
        for f in fields:
            assert got[f].tobytes() == s["fetch"][f].tobytes(), (fields, f)
        got = m.download_by_id(100, 777, fields)
        assert got.pop("present") == 777
        for f in fields:
            assert got[f].tobytes() == s["by_id"][f][100:877].tobytes(), (fields, f)


# ---- 2. the by-id download ---------------------------------------------------------------------------------------------------------------------
def test_download_by_id_is_the_multi_download_sorted_by_id(run40):
    world, m, states = run40
    assert N % 4 == 2  # (the 16-byte tail path of the one-tile run)
    for s in states:
        d, got = s["d"], s["by_id"]
        assert got["present"] == N and s["by_id2"]["present"] == N
        order = np.argsort(d["ids"], kind="stable")
        assert d["ids"][order].tolist() == list(range(N))
        for f in FLOATS:
            assert got[f].tobytes() == d[f][order].tobytes(), (s["what"], f)
            assert got[f].tobytes() == s["by_id2"][f].tobytes()
        check_answer(got, d, s["tiles"], np.arange(N, dtype=np.uint32), "%d tiles, by id, %s" % (world, s["what"]))
        assert got["tile"].tobytes() == s["by_id2"]["tile"].tobytes() and got["slot"].tobytes() == s["by_id2"]["slot"].tobytes()
        if world > 1:  # the window is larger than any tile's share
            assert np.bincount(got["tile"], minlength=world).max() < N
    # the state is the last one now: a window that starts mid-range and ends beyond N, an empty one, one beyond every id
    s = states[-1]
    first = N // 2 + 1
    ids = np.arange(first, first + N, dtype=np.uint32)
    got = m.download_by_id(first, N)
    assert got["present"] == N - first
    check_answer(got, s["d"], s["tiles"], ids, "a window beyond N")
    assert (got["tile"][N - first:] == A).all() and (bits(got["vel"])[N - first:] == W).all()
    got = m.download_by_id(17, 0)
    assert got["present"] == 0 and got["pos"].shape == (0, 2)
    got = m.download_by_id(2**32 - 8, 8)
    assert got["present"] == 0 and (got["slot"] == A).all() and (bits(got["density"]) == W).all()
    got = m.download_by_id(2**31 - 2, 4)  # (ids >= 2^31 are always absent: bit 31 is the owner bit)
    assert got["present"] == 0
    # after an unedited upload without ids: the particles in upload order (positions: the first state)
    assert states[0]["by_id"]["pos"].tobytes() == POS.astype(F).tobytes()
    # count=None: up to the largest id
    assert m.download_by_id()["pos"].tobytes() == states[-1]["by_id"]["pos"].tobytes()


def test_a_tile_without_particles_and_the_tail_of_the_array():
    """three strips along x, the third one to the right of the fluid (cells >= 5100: x >= 2.0; the column ends at x = 0.59), no
    re-partitioning: it owns nothing.  Its pass returns no record and the answer is complete."""
    m = make_multi(3, rebalance_every=0, strips=(0, [0, 5017, 5100, 65536]))
    m.steps(y.TimeManager(), 5)
    d, tiles = m.download(), tile_downloads(m)
    owned = [int(((t["ids"] >> 31) == 1).sum()) for t in tiles]
    print("local counts", [len(t["ids"]) for t in tiles], "owned", owned)
    assert owned[2] == 0 and owned[0] > 0 and owned[1] > 0
    got = m.download_by_id(0, N + 3)
    assert got["present"] == N and not (got["tile"] == 2).any()
    check_answer(got, d, tiles, np.arange(N + 3, dtype=np.uint32), "3 strips, one empty")
    ids, _ = id_set(tiles)
    m.track(ids)
    check_answer(m.track_fetch(), d, tiles, ids, "3 strips, one empty, fetch")
    # the tile-level seam on the empty tile: a window pass with room for no record returns none
    tc, n = m.tile_context(2), C.c_uint32(9)
    buf = np.full(4, 7, np.uint32)
    assert m.L.sphx_tile_track_window_enqueue(tc.h, 0, N, 0) == _lib.OK
    assert m.L.sphx_tile_track_window_fetch(tc.h, buf.ctypes.data, C.byref(n)) == _lib.OK and n.value == 0 and buf[0] == 0
    # a buffer smaller than what a tile owns: nothing is written past it and the call says so
    tc0 = m.tile_context(0)
    cap = 10
    buf = np.full(4 + 8 * cap + 8, 0xABABABAB, np.uint32)
    assert m.L.sphx_tile_track_window_enqueue(tc0.h, 0, N, cap) == _lib.OK
    assert m.L.sphx_tile_track_window_fetch(tc0.h, buf.ctypes.data, C.byref(n)) == _lib.ERR_CAPACITY and n.value == cap
    assert buf[0] == owned[0] and (buf[4 + 8 * cap:] == 0xABABABAB).all()
    own_ids = tiles[0]["ids"][(tiles[0]["ids"] >> 31) == 1] & ~OWNED
    rec = buf[4:4 + 8 * cap].reshape(cap, 8)
    assert len(set(rec[:, 0].tolist())) == cap and np.isin(rec[:, 0], own_ids).all() and (rec[:, 7] == 0).all()
    for r in rec:  # each stored record is the tile's own row at its slot
        assert tiles[0]["ids"][r[1]] == (r[0] | OWNED) and bits(tiles[0]["pos"][r[1]]).tolist() == r[2:4].tolist()
        assert bits(tiles[0]["vel"][r[1]]).tolist() == r[4:6].tolist() and bits(tiles[0]["density"])[r[1]] == r[6]
    assert m.download_by_id(0, N)["present"] == N  # (the multi call sizes its buffers itself)
    m.close()


# ---- 3. the recorder -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [1, 2, 4], ids=["one tile", "2 strips", "2x2"])
def test_recorder_through_simulation_steps(world):
    ids = np.concatenate([np.arange(N), [3, 3, N + 7, 2**31 + 2]]).astype(np.uint32)  # every particle: whoever migrates is in the set
    a = make_multi(world)
    assert a.track_status() == STATUS0
    a.track(ids)
    a.track_record(3, every=3)
    assert a.track_status() == dict(m=len(ids), recording=1, max_frames=3, every=3, frames=0, dropped=0)
    a.steps(y.TimeManager(), 12)  # (sphx_multi_simulation_steps: the frames are taken inside the library)
    assert a.track_status() == dict(m=len(ids), recording=1, max_frames=3, every=3, frames=3, dropped=1)
    frames, ftile = a.track_frames(tiles=True)
    assert frames.shape == (3, len(ids), 4) and ftile.shape == (3, len(ids))
    # an identical second run, stepped one at a time, fetched at steps 3, 6 and 9
    b = make_multi(world)
    b.track(ids)
    timer = y.TimeManager()
    for k in range(1, 10):
        b.step(timer)
        if k % 3 == 0:
            f = b.track_fetch()
            want = np.concatenate([bits(f["pos"]), bits(f["vel"])], axis=1)
            assert np.array_equal(bits(frames[k // 3 - 1]), want), "frame %d differs from the fetch at step %d" % (k // 3 - 1, k)
            assert np.array_equal(ftile[k // 3 - 1], f["tile"])
    assert (ftile[:, :N] < world).all() and (ftile[:, N + 2:] == A).all() and (bits(frames)[:, N + 2:] == W).all()
    assert np.array_equal(ftile[:, 3], ftile[:, N]) and np.array_equal(bits(frames[:, 3]), bits(frames[:, N + 1]))
    if world > 1:
        assert (ftile[0] != ftile[2]).any(), "no id changed its tile between the frames"
    part, ptile = a.track_frames(1, 2, tiles=True)
    assert part.tobytes() == frames[1:].tobytes() and ptile.tobytes() == ftile[1:].tobytes()
    assert a.track_frames(1, 2).tobytes() == part.tobytes() and a.track_frames(3, 0).shape == (0, len(ids), 4)
    assert "beyond the frames recorded" in refused(_lib.ERR_INVALID_ARGUMENT, a.track_frames, 2, 2)
    # the recording survives an upload; the set keeps its numbers
    a.upload(POS)
    assert a.track_status()["frames"] == 3 and a.track_status()["recording"] == 1 and a.track_fetch(("tile",))["tile"][0] != A
    # a new set discards the recording; max_frames == 0 stops
    a.track_record(2)
    a.track(ids[:10])
    assert a.track_status() == dict(m=10, recording=0, max_frames=0, every=0, frames=0, dropped=0)
    a.track_record(2)
    a.step(y.TimeManager())
    assert a.track_status()["frames"] == 1
    a.track_record(0, every=0)
    assert a.track_status() == dict(m=10, recording=0, max_frames=0, every=0, frames=0, dropped=0)
    a.track([])
    assert a.track_status() == STATUS0 and a.track_fetch()["pos"].shape == (0, 2)
    a.close(), b.close()


# ---- 4. every tiling sees the same particles -----------------------------------------------------------------------------------------------------
def test_2x2_against_the_single_context_in_tiling_invariant_mode():
    """2 x 2 tiles and the single context in tiling-invariant mode, fixed 2 + 2 iterations, 10 steps: the same particle set bit for bit,
    so the tiled fetch and by-id download are the single context's for pos, vel and density"""
    params = y.default_params(fixed_iterations=(2, 2))
    ctx = y.SphxContext(params)
    ctx.set_tiling_invariant(True)
    ctx.set_boundary(BOUNDARY)
    ctx.upload(POS)
    timer = y.TimeManager()
    for _ in range(10):
        vmax = ctx.step_begin(timer.simulation_step(), timer.law(F(0.01)))
        ctx.step_finish(y.duration_as_secs_f32(timer.update_simulation_step(F(0.01), vmax)))
    m = make_multi(4, params=y.default_params(fixed_iterations=(2, 2)), invariant=True)
    t2 = y.TimeManager()
    m.steps(t2, 10)
    assert t2.simulation_step_ns() == timer.simulation_step_ns()
    ids, _ = id_set(tile_downloads(m))
    ctx.track(ids)
    m.track(ids)
    single, tiled = ctx.track_fetch(), m.track_fetch()
    for f in FLOATS:
        assert single[f].tobytes() == tiled[f].tobytes(), f
    assert np.array_equal(single["slot"] == A, tiled["tile"] == A)
    single, tiled = ctx.download_by_id(50, N), m.download_by_id(50, N)
    assert single["present"] == tiled["present"] == N - 50
    for f in FLOATS:
        assert single[f].tobytes() == tiled[f].tobytes(), f
    ctx.close()
    m.close()


# ---- 5. edits --------------------------------------------------------------------------------------------------------------------------------
def test_removed_ids_become_absent_and_appended_ids_are_found():
    m = make_multi(4)
    m.steps(y.TimeManager(), 6)
    new = np.array([[0.70, 1.15], [0.72, 1.15], [0.70, 1.17]], F)  # in the air beside the column
    ids = np.concatenate([np.arange(0, N, 3), [N, N + 1, N + 2, N + 3]]).astype(np.uint32)  # (N .. N + 2 are announced before they exist)
    m.track(ids)
    m.track_record(4)
    before, d0 = m.track_fetch(), m.download()
    assert (before["tile"][-4:] == A).all()
    p = d0["pos"]
    qx, qy = np.quantile(p[:, 0], [0.3, 0.6]), np.quantile(p[:, 1], [0.3, 0.6])
    hole = (float(qx[0]), float(qy[0]), float(qx[1]), float(qy[1]))
    removed = m.remove(hole)
    assert removed > 0
    d, tiles = m.download(), tile_downloads(m)
    assert len(d["ids"]) == N - removed
    after = m.track_fetch()
    present = check_answer(after, d, tiles, ids, "after the removal")
    gone = ~present[:-4]
    bp = before["pos"][:-4]
    closed = (bp[:, 0] >= hole[0]) & (bp[:, 0] <= hole[2]) & (bp[:, 1] >= hole[1]) & (bp[:, 1] <= hole[3])
    inside = (bp[:, 0] > hole[0]) & (bp[:, 0] < hole[2]) & (bp[:, 1] > hole[1]) & (bp[:, 1] < hole[3])
    assert gone.any() and not gone.all() and closed[gone].all() and gone[inside].all()  # exactly the tracked ids inside the rectangle
    for f in ("pos", "vel"):  # the others are unchanged
        assert np.array_equal(bits(after[f])[:-4][~gone], bits(before[f])[:-4][~gone]), f
    first = m.append(new)
    assert first == N
    d, tiles = m.download(), tile_downloads(m)
    got = m.track_fetch()
    present = check_answer(got, d, tiles, ids, "after the append")
    assert present[-4:].tolist() == [True, True, True, False]
    assert bits(got["pos"][-4:-1]).tolist() == bits(new).tolist()
    by_id = m.download_by_id(0, N + 4)
    assert by_id["present"] == N - removed + 3
    check_answer(by_id, d, tiles, np.arange(N + 4, dtype=np.uint32), "by id after the edits")
    # the set and the recording have survived both edits, and a checkpoint loaded into the run
    assert m.track_status() == dict(m=len(ids), recording=1, max_frames=4, every=1, frames=0, dropped=0)
    m.step(y.TimeManager())
    blob = m.save_state()
    m.load_state(blob)
    assert m.track_status()["frames"] == 1 and m.track_status()["m"] == len(ids)
    check_answer(m.track_fetch(), m.download(), tile_downloads(m), ids, "after a state load")
    m.close()


# ---- 6. no side effects -------------------------------------------------------------------------------------------------------------------------
def test_a_run_with_tracking_is_bit_identical_to_the_run_without():
    steps = 20

    def run(observed):
        m = make_multi(4)
        if observed:
            m.track(np.arange(0, N, 2, dtype=np.uint32))
            m.track_record(steps // 2, every=2)
        timer = y.TimeManager()
        out = []
        for k in range(steps):
            out.append(m.step(timer))
            if observed and k % 2:
                m.track_fetch()
                m.download_by_id(0, N)
                m.track_frames()
        if observed:
            assert m.track_status()["frames"] == steps // 2
        dig, info, ns = m.state_digest(), m.info(), (timer.simulation_step_ns(), timer.total_simulated_ns, timer.num_steps)
        m.close()
        return dig, out, info, ns

    da, sa, ia, ta = run(False)
    db, sb, ib, tb = run(True)
    assert da == db and len(da) == len(_lib.MULTI_STATE_SECTIONS)
    for k, (a, b) in enumerate(zip(sa, sb)):
        for f in STEP_FIELDS + ("dt_ns",):
            assert np.array(a[f]).tobytes() == np.array(b[f]).tobytes(), (k, f, a[f], b[f])
    assert ta == tb
    assert ia["exchanges"] == ib["exchanges"] and ia["rebalances"] == ib["rebalances"] and ia["halo_now"] == ib["halo_now"]


# ---- 8. state rules and argument errors -----------------------------------------------------------------------------------------------------------
def test_state_rules_and_argument_errors():
    bad, not_ready = _lib.ERR_INVALID_ARGUMENT, _lib.ERR_NOT_READY
    m = new_multi(2)
    # before the first upload
    for fn, args in ((m.track, ([1, 2],)), (m.track_fetch, ()), (m.track_record, (4,)), (m.track_frames, ()), (m.download_by_id, (0, 4))):
        assert "before the first" in refused(not_ready, fn, *args)
    assert m.track_status() == STATUS0
    m.upload(POS)
    L, h = m.L, m.h

    def err(rc, code, needle):
        msg = L.sphx_multi_last_error(h).decode()
        assert rc == code and needle in msg, (rc, msg)

    buf = np.zeros(64, np.float32)
    til = np.zeros(32, np.uint32)
    o = _lib.SphxMultiTrackOut(til.ctypes.data, None, buf.ctypes.data, None, None)
    none = _lib.SphxMultiTrackOut()
    ids = np.arange(_lib.TRACK_MAX_IDS + 1, dtype=np.uint32)
    err(L.sphx_multi_track_set(h, ids.ctypes.data, len(ids)), bad, "SPHX_TRACK_MAX_IDS")
    err(L.sphx_multi_track_set(h, None, 3), bad, "ids")
    err(L.sphx_multi_track_record(h, 4, 1), not_ready, "empty")  # recording with an empty set
    assert L.sphx_multi_track_fetch(h, 0, C.byref(o)) == _lib.OK  # (an empty set: a successful no-op)
    assert L.sphx_multi_track_set(h, ids.ctypes.data, 8) == _lib.OK
    err(L.sphx_multi_track_fetch(h, 0, None), bad, "out")
    err(L.sphx_multi_track_fetch(h, 0, C.byref(none)), bad, "every pointer")
    err(L.sphx_multi_track_fetch(h, 1, C.byref(o)), bad, "flags")
    err(L.sphx_multi_download_by_id(h, 0, 8, 0, None, None), bad, "out")
    err(L.sphx_multi_download_by_id(h, 0, 8, 0, C.byref(none), None), bad, "every pointer")
    err(L.sphx_multi_download_by_id(h, 0, 8, 0x80000000, C.byref(o), None), bad, "flags")
    err(L.sphx_multi_download_by_id(h, 2**32 - 4, 5, 0, C.byref(o), None), bad, "2^32")
    err(L.sphx_multi_track_record(h, 4, 0), bad, "every")
    err(L.sphx_multi_track_record(h, (1 << 30) // (8 * 20) + 1, 1), _lib.ERR_CAPACITY, "1 GiB")
    err(L.sphx_multi_track_read(h, 0, 1, 0, buf.ctypes.data, None), bad, "beyond the frames recorded")
    err(L.sphx_multi_track_read(h, 0, 0, 1, buf.ctypes.data, None), bad, "flags")
    assert L.sphx_multi_track_get_status(h, None) == bad
    assert not buf.any() and not til.any()  # a refused call writes nothing
    assert m.track_status() == dict(m=8, recording=0, max_frames=0, every=0, frames=0, dropped=0)  # ... and touches no tile
    assert L.sphx_multi_download_by_id(h, 2**32 - 4, 4, 0, C.byref(o), None) == _lib.OK and til[:4].tolist() == [A] * 4
    m.track_record(2)
    m.step(y.TimeManager())
    err(L.sphx_multi_track_read(h, 0, 1, 0, None, None), bad, "out")
    err(L.sphx_multi_track_read(h, 1, 1, 0, buf.ctypes.data, None), bad, "beyond the frames recorded")
    assert L.sphx_multi_track_read(h, 0, 1, 0, buf.ctypes.data, None) == _lib.OK  # (out_tile may be NULL)
    # inside an open multi step
    timer = y.TimeManager()
    vmax = m.step_begin(y.duration_as_secs_f32(timer.simulation_step_ns()))
    for fn, args in ((m.track, ([1, 2],)), (m.track_fetch, ()), (m.track_record, (4,)), (m.track_frames, ()), (m.download_by_id, (0, 4))):
        assert "sphx_multi_step_begin" in refused(not_ready, fn, *args)
    m.step_finish(y.duration_as_secs_f32(timer.update_simulation_step(F(0.01), vmax)))
    assert m.track_status()["frames"] == 2 and m.track_fetch()["tile"].tolist() != [A] * 8
    # one tile: the single-context family keeps refusing a tile, the tile calls refuse a plain context
    tc = m.tile_context(0)
    assert "tile context" in refused(bad, tc.track, [1])
    assert "tile context" in refused(bad, tc.download_by_id, 0, 4)
    plain = y.SphxContext()
    plain.set_boundary(BOUNDARY)
    plain.upload(POS)
    n = C.c_uint32()
    assert L.sphx_tile_track_install(plain.h, ids.ctypes.data, ids.ctypes.data, 4, 10) == bad and "not a tile context" in L.sphx_last_error(plain.h).decode()
    assert L.sphx_tile_track_fetch_enqueue(plain.h) == bad and L.sphx_tile_track_window_enqueue(plain.h, 0, 4, 4) == bad
    assert L.sphx_tile_track_window_fetch(plain.h, til.ctypes.data, C.byref(n)) == bad and L.sphx_tile_track_record(plain.h, 2, 1) == bad
    assert L.sphx_tile_track_frame(plain.h) == bad and L.sphx_tile_track_read(plain.h, 0, 0, None, None) == bad
    assert L.sphx_tile_track_fetch(plain.h, til.ctypes.data, buf.ctypes.data, buf.ctypes.data) == bad
    assert L.sphx_tile_track_window_enqueue(tc.h, 0, (1 << 22) + 1, 4) == bad
    plain.track([1, 2])
    assert plain.track_fetch()["slot"].tolist() != [A, A]
    plain.close()
    m.close()


# ---- 9. the solver object -------------------------------------------------------------------------------------------------------------------------
def test_solver_object_reaches_the_tiled_tracking():
    w = y.FluidParticleWorld()
    w.reset_fluid(1.0)
    s = y.DFSPHMultiSolver(w, [0, 0])
    t = y.TimeManager()
    assert "before the first" in refused(_lib.ERR_NOT_READY, s.track, [1, 2])  # (the solver uploads with its first step)
    assert s.track_status()["m"] == 0
    s.simulation_step(w, t, sync_world=False)
    n = len(w.positions)
    ids = np.array([0, n - 1, n // 2, n // 2, n + 9], np.uint32)
    s.track(ids)
    s.track_record(4, every=2)
    s.simulation_steps(w, t, 4, sync_world=True)
    assert s.track_status() == dict(m=5, recording=1, max_frames=4, every=2, frames=2, dropped=0)
    frames, tiles = s.track_frames(tiles=True)
    got = s.track_fetch()
    d, td = s.multi().download(), tile_downloads(s.multi())
    check_answer(got, d, td, ids, "the solver object's tiles")
    assert np.array_equal(bits(frames[1]), np.concatenate([bits(got["pos"]), bits(got["vel"])], axis=1)) and np.array_equal(tiles[1], got["tile"])
    by_id = s.download_by_id(0, n)
    assert by_id["present"] == n
    order = np.argsort(np.asarray(w.particle_ids), kind="stable")
    assert by_id["pos"].tobytes() == np.ascontiguousarray(np.asarray(w.positions)[order], F).tobytes()
    s.close()


# ---- 10. one process per tile -------------------------------------------------------------------------------------------------------------------------
def test_rank_mode_parts_fold_to_the_in_process_run(tmp_path):
    """Two processes over gloo (the halo records) and the shared segment (the scalars).  The tracking calls are local: each rank writes
    its part; the parts, folded with track_merge / track_merge_frames, are the bytes of the in-process devices=[0, 0] run."""
    steps, every = 12, 3
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1", "--master-port", "29553",
           os.path.join(HERE, "track_multi_rank_worker.py"), str(tmp_path), str(steps), str(every)]
    p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    r = [np.load(tmp_path / f"rank{k}.npz") for k in range(2)]
    ids = r[0]["ids"]
    assert np.array_equal(ids, r[1]["ids"]) and np.array_equal(r[0]["status"], r[1]["status"])
    m = make_multi(2)
    m.track(ids)
    m.track_record(16, every=every)
    m.steps(y.TimeManager(), steps)
    assert r[0]["status"].tolist() == [m.track_status()[k] for k in ("m", "recording", "max_frames", "every", "frames", "dropped")]
    for prefix, want in (("fetch_", m.track_fetch()), ("byid_", m.download_by_id(0, N + 5))):
        parts = [{f: (r[k][prefix + f].view(F) if f in FLOATS else r[k][prefix + f]) for f in y.MULTI_TRACK_FIELDS} for k in range(2)]
        # a rank's part holds only what it owns, under its own rank
        for k in range(2):
            on = parts[k]["tile"] != A
            assert (parts[k]["tile"][on] == k).all() and on.any() and not on.all()
        assert not ((parts[0]["tile"] != A) & (parts[1]["tile"] != A)).any()
        got = y.track_merge(parts)
        present = got.pop("present")
        assert present == int((want["tile"] != A).sum())
        if prefix == "byid_":
            assert present == N == want["present"] == int(r[0]["present"][0]) + int(r[1]["present"][0])
        for f in y.MULTI_TRACK_FIELDS:
            assert got[f].tobytes() == want[f].tobytes(), (prefix, f)
    frames, tiles = m.track_frames(tiles=True)
    got_f, got_t = y.track_merge_frames([(r[k]["frames"].view(F), r[k]["frame_tiles"]) for k in range(2)])
    assert frames.shape == (steps // every, len(ids), 4) and got_f.tobytes() == frames.tobytes() and got_t.tobytes() == tiles.tobytes()
    m.close()
