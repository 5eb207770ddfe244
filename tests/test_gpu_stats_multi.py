"""Fluid statistics of a tiled run on the device (include/sphx.h, "fluid statistics of a tiled run"): sphx_multi_fluid_stats, the multi
recorder and sphx_tile_fluid_stats against tests/stats_reference.py.  The truth is always computed from what sphx_multi_download returns:
counts, extremes and max_speed_sq bit for bit, every sum against the stated bound n * 2^-52 * fsum(|t|).  All scenes are the dam break
of tests/util.py at scale 1.0 (4 050 particles, every tile on device 0): small, and it has ghosts, migration, re-partitioning and empty
regions.  The exports, the NULL refusals and the host side of the fold are checked without a GPU in tests/test_stats_multi_host.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

import stats_reference as ref
import yasph2d_amd as y
from tiles_reference import cell_coord
from util import dam_break
from yasph2d_amd import _lib
from yasph2d_amd.multi import MultiSolver

pytestmark = pytest.mark.gpu

F = np.float32
INF = float("inf")
HERE = os.path.dirname(os.path.abspath(__file__))
EVERYTHING = (-INF, -INF, INF, INF)
NOWHERE = (5.0, 5.0, 6.0, 6.0)  # inside the domain, far from the fluid: no tile holds a particle there
POS, BOUNDARY = dam_break(1.0)
N = len(POS)
STEP_FIELDS = tuple(k for k, _ in _lib.SphxStepStats._fields_)  # every sphx_step_stats field


def refused(code, fn, *args, **kw):
    with pytest.raises(y.SphxError) as e:
        fn(*args, **kw)
    assert e.value.code == code, str(e.value)
    return str(e.value)


def make_multi(world, params=None, rebalance_every=4, halo=10, strips=None, invariant=False):
    m = MultiSolver(params if params is not None else y.default_params(), devices=[0] * world, halo=halo, rebalance_every=rebalance_every)
    if invariant:
        m.set_tiling_invariant(True)
    if strips is not None:
        m.set_strips(*strips)
    m.set_boundary(BOUNDARY)
    m.upload(POS)
    return m


def rects_of(d):
    """eight rectangles on a downloaded state: two wide bands through the middle of the fluid (they straddle the cuts, which sit near the
    particle-count quantiles), a box, an empty region, an inverted one, infinite and half-infinite bounds, a small box round a particle"""
    p = d["pos"]
    qx = [float(v) for v in np.quantile(p[:, 0], [0.1, 0.25, 0.5, 0.6, 0.75])]
    qy = [float(v) for v in np.quantile(p[:, 1], [0.1, 0.25, 0.5, 0.6, 0.75])]
    c = p[len(p) // 3]
    return [(qx[1], -INF, qx[4], INF), (-INF, qy[1], INF, qy[4]), (qx[0], qy[0], qx[3], qy[3]), NOWHERE, (qx[4], qy[1], qx[1], qy[4]), EVERYTHING,
            (-INF, qy[2], qx[2], INF), (float(c[0]) - 0.02, float(c[1]) - 0.02, float(c[0]) + 0.02, float(c[1]) + 0.02)]


def check_all(got, d, rects, what, density_valid=True, slack=1.0):
    """every record of one call against the reference over the particles d; each figure of a sum is printed before it is judged"""
    want = ref.stats(d, rects, density_valid)
    assert got.dtype == y.STATS_DTYPE and got.shape == (1 + len(rects),)
    for r, (g, w) in enumerate(zip(got, want)):
        for k in ref.SUMS:
            gs, ws, ab = np.atleast_1d(g[k]), np.atleast_1d(w[k]), np.atleast_1d(w["abs_" + k])
            for j in range(len(gs)):
                print("%s record %d %s[%d]: device %.17g exact %.17g |diff| %.3g bound %.3g" % (
                    what, r, k, j, gs[j], ws[j], abs(float(gs[j]) - float(ws[j])), slack * w["n_" + k] * ref.U * ab[j]))
        ref.check(g, w, "%s, record %d" % (what, r), slack)
    return want


def subset(d, sel):
    return {k: v[sel] for k, v in d.items()}


# ---- a Python restatement of a (+) b and of the fold in ascending tile rank (sphx_stats_merge.hpp) --------------------------------------------
def _key(f):
    i = int(np.array([f], F).view(np.int32)[0])
    return i ^ ((i >> 31) & 0x7FFFFFFF)


def _kmin(a, b):
    return a if _key(a) < _key(b) else b


def _kmax(a, b):
    return a if _key(a) > _key(b) else b


def merge(a, b):
    r = np.zeros(1, y.STATS_DTYPE)[0]
    for k in ("count", "nonfinite", "density_count"):
        r[k] = a[k] + b[k]
    r["density_valid"] = int(bool(a["density_valid"]) and bool(b["density_valid"]))
    for k in ref.SUMS:
        r[k] = np.asarray(a[k], np.float64) + np.asarray(b[k], np.float64)
    r["max_speed_sq"] = max(float(a["max_speed_sq"]), float(b["max_speed_sq"]))
    for j in range(2):
        r["min_pos"][j] = _kmin(a["min_pos"][j], b["min_pos"][j])
        r["max_pos"][j] = _kmax(a["max_pos"][j], b["max_pos"][j])
    r["min_density"], r["max_density"] = _kmin(a["min_density"], b["min_density"]), _kmax(a["max_density"], b["max_density"])
    return r


def fold(tiles):
    """tiles [world, nrec] -> [nrec]"""
    out = tiles[0].copy()
    for t in range(1, len(tiles)):
        for r in range(len(out)):
            out[r] = merge(out[r], tiles[t][r])
    return out


def tile_boxes(m, world):
    """the cell box of what each tile owns, from the tiles' own sphx_download (owned = bit 31 of the id): the tiles' rectangles as far as
    the particles can tell"""
    boxes = []
    for k in range(world):
        t = m.tile_context(k).download()
        own = (t["ids"] >> 31) == 1
        if not own.any():
            boxes.append(None)
            continue
        cx, cy = cell_coord(t["pos"][own], 0), cell_coord(t["pos"][own], 1)
        boxes.append((int(cx.min()), int(cx.max()), int(cy.min()), int(cy.max())))
    return boxes


# ---- 1 + 2. the whole fluid and the tiles' own records -------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[1, 2, 4], ids=["one tile", "2 strips", "2x2"])
def run40(request):
    """after the upload and after 40 adaptive steps with a re-partition every 4: (world, multi, [(what, download, rects, whole, tiles)])"""
    world = request.param
    m = make_multi(world)
    states = []
    d = m.download()
    rects = rects_of(d)
    states.append(("after the upload",) + (d, rects) + m.stats(rects, per_tile=True))
    timer = y.TimeManager()
    m.steps(timer, 40)
    d = m.download()
    rects = rects_of(d)
    states.append(("after 40 steps",) + (d, rects) + m.stats(rects, per_tile=True))
    if world > 1:
        assert m.info()["rebalances"] >= 1, m.info()
    yield world, m, states
    m.close()


def test_whole_fluid_against_the_reference(run40):
    world, m, states = run40
    for what, d, rects, whole, tiles in states:
        assert len(d["ids"]) == N and len(rects) == 8
        want = check_all(whole, d, rects, "%d tiles, %s" % (world, what))
        assert whole[0]["count"] == N and whole[6]["count"] == N and (whole["density_valid"] == 1).all() and (whole["reserved"] == 0).all()
        assert whole[4]["count"] == 0 and whole[5]["count"] == 0 and whole[4]["min_pos"].tolist() == [INF, INF]  # the empty region, the inverted one
        assert all(0 < whole[r]["count"] < N for r in (1, 2, 3, 7, 8))
        assert want[0]["sum_density"] > 0 and whole[0]["density_count"] == N
        if world > 1:  # the two bands straddle a tile border: more than one tile holds particles of theirs
            assert (tiles[:, 1]["count"] > 0).sum() >= 2 and (tiles[:, 2]["count"] > 0).sum() >= (2 if world == 4 else 1)


def test_per_tile_records(run40):
    world, m, states = run40
    what, d, rects, whole, tiles = states[-1]
    assert tiles.shape == (world, 9)
    assert int(tiles[:, 0]["count"].sum()) == N == m.L.sphx_multi_num_owned(m.h) == whole[0]["count"]
    # each tile's records = the reference over the downloaded particles whose cell lies in that tile's rectangle
    boxes = tile_boxes(m, world)
    cx, cy = cell_coord(d["pos"], 0), cell_coord(d["pos"], 1)
    member = np.zeros((world, N), bool)
    for k, b in enumerate(boxes):
        if b is not None:
            member[k] = (cx >= b[0]) & (cx <= b[1]) & (cy >= b[2]) & (cy <= b[3])
    assert (member.sum(axis=0) == 1).all(), "the tiles' cell boxes do not partition the fluid"
    for k in range(world):
        check_all(tiles[k], subset(d, member[k]), rects, "%d tiles, tile %d" % (world, k))
        assert tiles[k][0]["count"] == member[k].sum()
    assert (tiles[:, 0]["count"] > 0).all()
    # the fold of out_tiles in ascending rank, restated in Python, is `out` bit for bit
    assert fold(tiles).tobytes() == whole.tobytes()
    # and one tile alone: the tile-level call returns that tile's row
    for k in range(world):
        assert m.tile_context(k).tile_stats(rects).tobytes() == tiles[k].tobytes()


# ---- 3. a tile that owns nothing ---------------------------------------------------------------------------------------------------------------
def test_a_tile_without_particles_returns_the_empty_record():
    """three strips along x, the third one to the right of the fluid (cells >= 5100: x >= 2.0; the column ends at x = 0.59), no
    re-partitioning: after a few steps it still owns nothing"""
    m = make_multi(3, rebalance_every=0, strips=(0, [0, 5017, 5100, 65536]))
    timer = y.TimeManager()
    m.steps(timer, 5)
    d = m.download()
    rects = [EVERYTHING, NOWHERE, (0.3, 0.9, 0.5, 1.2)]
    whole, tiles = m.stats(rects, per_tile=True)
    assert tiles[:, 0]["count"].tolist()[2] == 0 and tiles[0][0]["count"] > 0 and tiles[1][0]["count"] > 0
    empty = ref.stats((np.zeros((0, 2), F), np.zeros((0, 2), F), np.zeros(0, F)), rects, True)
    for r in range(4):
        ref.check(tiles[2][r], empty[r], "the empty tile, record %d" % r)
        assert tiles[2][r]["min_pos"].tolist() == [INF, INF] and tiles[2][r]["max_density"] == -INF and tiles[2][r]["density_valid"] == 1
        for k in ref.SUMS:
            assert ref.bits(tiles[2][r][k]) == ref.bits(np.zeros_like(np.atleast_1d(tiles[2][r][k])))  # +0, not -0
    check_all(whole, d, rects, "3 strips, one empty")
    assert whole[2]["count"] == 0 and (tiles[:, 2]["count"] == 0).all()  # a rectangle no tile intersects
    assert fold(tiles).tobytes() == whole.tobytes()
    assert m.tile_context(2).tile_stats(rects).tobytes() == tiles[2].tobytes()
    m.close()


# ---- 4. every tiling sees the same fluid ---------------------------------------------------------------------------------------------------------
def test_2x2_against_the_single_context_in_tiling_invariant_mode():
    """2 x 2 tiles and the single context in tiling-invariant mode, fixed 2 + 2 iterations, 10 steps: the same particle set bit for bit, so
    counts, extremes, max_speed_sq and density_valid are identical and each pair of sums differs by at most twice the bound"""
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
    d = m.download()
    rects = rects_of(d)
    single, tiled = ctx.stats(rects), m.stats(rects)
    want = ref.stats(d, rects, True)
    for r in range(9):
        for k in ref.EXACT:
            assert ref.bits(single[r][k]) == ref.bits(tiled[r][k]), (r, k, single[r][k], tiled[r][k])
        for k in ref.SUMS:
            a, b, ab = np.atleast_1d(single[r][k]), np.atleast_1d(tiled[r][k]), np.atleast_1d(want[r]["abs_" + k])
            for j in range(len(a)):
                bound = 2.0 * want[r]["n_" + k] * ref.U * ab[j]
                print("record %d %s[%d]: single %.17g tiled %.17g |diff| %.3g bound %.3g" % (r, k, j, a[j], b[j], abs(float(a[j]) - float(b[j])), bound))
                assert abs(float(a[j]) - float(b[j])) <= bound, (r, k, j)
    assert tiled[0]["count"] == N and tiled[0]["density_valid"] == 1
    ctx.close()
    m.close()


# ---- 5. determinism ------------------------------------------------------------------------------------------------------------------------------
def test_two_calls_are_identical_and_a_frame_equals_the_call_of_its_step():
    m = make_multi(4)
    rects = rects_of(m.download())
    m.stats_record(rects, 6)
    timer = y.TimeManager()
    calls = []
    for _ in range(6):
        m.step(timer)
        a, ta = m.stats(rects, per_tile=True)
        b, tb = m.stats(rects, per_tile=True)
        assert a.tobytes() == b.tobytes() and ta.tobytes() == tb.tobytes()
        calls.append(a)
    rec, info = m.stats_frames()
    assert rec.shape == (6, 9) and info["step"].tolist() == [1, 2, 3, 4, 5, 6]
    for k in range(6):
        assert rec[k].tobytes() == calls[k].tobytes(), "frame %d differs from the call made at that step" % k
    assert m.stats(rects).tobytes() == calls[-1].tobytes()  # (reading the frames changed nothing)
    m.close()


# ---- 6. the recorder -------------------------------------------------------------------------------------------------------------------------------
def test_recorder_through_simulation_steps():
    m = make_multi(2)
    L = m.L
    rects = [EVERYTHING, (0.0, 0.0, 0.35, 1.2)]
    assert m.stats_status() == dict(n_rects=0, recording=0, max_frames=0, every=0, frames=0, dropped=0)
    m.stats_record(rects, 3, every=3)
    assert m.stats_status() == dict(n_rects=2, recording=1, max_frames=3, every=3, frames=0, dropped=0)
    timer = y.TimeManager()
    steps = m.steps(timer, 12)  # (sphx_multi_simulation_steps: the frames are taken inside the library)
    assert m.stats_status() == dict(n_rects=2, recording=1, max_frames=3, every=3, frames=3, dropped=1)
    rec, info = m.stats_frames()
    assert rec.shape == (3, 3) and info["step"].tolist() == [3, 6, 9] and info["n"].tolist() == [N] * 3
    assert info["dt"].tolist() == [F(steps[k]["dt"]) for k in (2, 5, 8)]
    assert (rec[:, 0]["count"] == N).all() and (rec["density_valid"] == 1).all()
    part, pinfo = m.stats_frames(1, 2)
    assert part.tobytes() == rec[1:].tobytes() and pinfo.tobytes() == info[1:].tobytes()
    assert m.stats_frames(3, 0)[0].shape == (0, 3)
    msg = refused(_lib.ERR_INVALID_ARGUMENT, m.stats_frames, 2, 2)  # a read beyond `frames`
    assert "beyond the frames recorded" in msg
    # a new recording discards the old one and counts from its own call
    m.stats_record([], 8, every=3)
    assert m.stats_status() == dict(n_rects=0, recording=1, max_frames=8, every=3, frames=0, dropped=0)
    more = m.steps(timer, 12)
    rec, info = m.stats_frames()
    assert rec.shape == (4, 1) and info["step"].tolist() == [3, 6, 9, 12] and info["dt"].tolist() == [F(more[k]["dt"]) for k in (2, 5, 8, 11)]
    d = m.download()
    check_all(rec[3], d, [], "the frame of the last step")
    assert rec[3].tobytes() == m.stats().tobytes()
    # the recording survives an upload
    m.upload(POS)
    assert m.stats_status()["frames"] == 4 and m.stats_status()["recording"] == 1
    timer = y.TimeManager()
    m.steps(timer, 3)
    assert m.stats_status()["frames"] == 5 and m.stats_frames(4, 1)[1]["step"].tolist() == [15]
    # limits
    big = (64 << 20) // 128 + 1
    assert "64 MiB" in refused(_lib.ERR_CAPACITY, m.stats_record, [], big)
    assert "64 MiB" in refused(_lib.ERR_CAPACITY, m.stats_record, [EVERYTHING] * 8, (64 << 20) // (9 * 128) + 1)
    assert "every" in refused(_lib.ERR_INVALID_ARGUMENT, m.stats_record, [], 4, every=0)
    assert m.stats_status()["frames"] == 5  # (a refused call leaves the recording alone)
    m.stats_record([], 0, every=0)  # stops and frees, whatever `every` says
    assert m.stats_status() == dict(n_rects=0, recording=0, max_frames=0, every=0, frames=0, dropped=0)
    refused(_lib.ERR_INVALID_ARGUMENT, m.stats_frames, 0, 1)
    m.steps(timer, 2)
    assert m.stats_status()["frames"] == 0
    st = _lib.SphxStatsStatus()
    assert L.sphx_multi_stats_get_status(m.h, None) == _lib.ERR_INVALID_ARGUMENT and L.sphx_multi_stats_get_status(m.h, st) == _lib.OK
    m.close()


# ---- 7. no side effects ----------------------------------------------------------------------------------------------------------------------------
def test_a_run_with_stats_is_bit_identical_to_the_run_without():
    """twin 2 x 2 runs of the dam break (the collapse of the column: warm starts, extra exchanges, migration), a re-partition every 4
    steps; one of them records a frame every step and is asked for statistics (whole fluid, per tile, one tile) after every second step"""
    steps = 150

    def run(observed):
        m = make_multi(4)
        rects = rects_of(m.download())
        if observed:
            m.stats_record(rects, steps)
        timer = y.TimeManager()
        out = []
        for k in range(steps):
            out.append(m.step(timer))
            if observed and k % 2:
                m.stats(rects, per_tile=True)
                m.tile_context(k % 4).tile_stats(rects[:3])
        if observed:
            assert m.stats_status()["frames"] == steps
            m.stats_frames()
        d, info = m.download(), m.info()
        m.close()
        return d, out, info

    da, sa, ia = run(False)
    db, sb, ib = run(True)
    for k in ("ids", "pos", "vel", "density"):
        assert da[k].tobytes() == db[k].tobytes(), k
    for k, (a, b) in enumerate(zip(sa, sb)):
        for f in STEP_FIELDS + ("dt_ns",):
            assert np.array(a[f]).tobytes() == np.array(b[f]).tobytes(), (k, f, a[f], b[f])
    assert len(STEP_FIELDS) == 12 and set(STEP_FIELDS) <= set(sa[0])
    assert ia["exchanges"] == ib["exchanges"] and ia["rebalances"] == ib["rebalances"] >= 3 and ia["halo_now"] == ib["halo_now"]


# ---- 8. state rules and argument errors ------------------------------------------------------------------------------------------------------------
def test_state_rules_and_argument_errors():
    m = make_multi(2)
    L, h, bad = m.L, m.h, _lib.ERR_INVALID_ARGUMENT
    rec = np.zeros(9, y.STATS_DTYPE)
    tiles = np.zeros((2, 2), y.STATS_DTYPE)  # [world][1 + n_rects] of the one-rectangle call below
    p = rec.ctypes.data
    one = (_lib.SphxRect * 1)(_lib.SphxRect(0, 0, 1, 1))
    many = (_lib.SphxRect * 9)()

    def err(rc, code, needle):
        msg = L.sphx_multi_last_error(h).decode()
        assert rc == code and needle in msg, (rc, msg)

    err(L.sphx_multi_fluid_stats(h, None, 0, 0, None, None), bad, "out")
    err(L.sphx_multi_fluid_stats(h, None, 1, 0, p, None), bad, "rects")
    err(L.sphx_multi_fluid_stats(h, many, 9, 0, p, None), bad, "SPHX_STATS_MAX_RECTS")
    for k in range(4):
        v = [0.0, 0.0, 1.0, 1.0]
        v[k] = float("nan")
        err(L.sphx_multi_fluid_stats(h, (_lib.SphxRect * 1)(_lib.SphxRect(*v)), 1, 0, p, None), bad, "NaN")
        err(L.sphx_multi_stats_record(h, (_lib.SphxRect * 1)(_lib.SphxRect(*v)), 1, 4, 1), bad, "NaN")
    err(L.sphx_multi_fluid_stats(h, one, 1, 1, p, None), bad, "flags")  # (there is no device-pointer path on this level)
    err(L.sphx_multi_fluid_stats(h, one, 1, 0x80000000, p, None), bad, "flags")
    err(L.sphx_multi_stats_record(h, None, 1, 4, 1), bad, "rects")
    err(L.sphx_multi_stats_record(h, many, 9, 4, 1), bad, "SPHX_STATS_MAX_RECTS")
    assert not rec.tobytes().strip(b"\0")  # a refused call writes nothing
    assert L.sphx_multi_fluid_stats(h, one, 1, 0, p, tiles.ctypes.data) == _lib.OK and rec[0]["count"] == N == tiles[:, 0]["count"].sum()
    assert L.sphx_multi_fluid_stats(h, None, 0, 0, p, None) == _lib.OK  # (rects may be NULL with n_rects == 0, out_tiles may be NULL)
    # inside an open multi step
    timer = y.TimeManager()
    vmax = m.step_begin(y.duration_as_secs_f32(timer.simulation_step_ns()))
    assert "sphx_multi_step_begin" in refused(_lib.ERR_NOT_READY, m.stats)
    refused(_lib.ERR_NOT_READY, m.stats_record, [], 4)
    refused(_lib.ERR_NOT_READY, m.stats_frames, 0, 0)
    m.step_finish(y.duration_as_secs_f32(timer.update_simulation_step(F(0.01), vmax)))
    whole, per = m.stats([EVERYTHING], per_tile=True)
    assert whole[0]["count"] == N
    # one tile: the tile-level call is that tile's row; the single-context family keeps refusing a tile, the tile call refuses a plain context
    for k in range(2):
        tc = m.tile_context(k)
        assert tc.tile_stats([EVERYTHING]).tobytes() == per[k].tobytes()
        assert "tile context" in refused(bad, tc.stats)
        assert "tile context" in refused(bad, tc.stats_record, [], 4)
        err2 = L.sphx_tile_fluid_stats(tc.h, one, 1, 2, p)
        assert err2 == bad and "flags" in L.sphx_last_error(tc.h).decode()
        assert L.sphx_tile_fluid_stats(tc.h, one, 1, _lib.STATS_DEVICE_POINTERS, p | 4) == bad
        assert L.sphx_tile_fluid_stats(tc.h, None, 0, 0, None) == bad
    plain = y.SphxContext()
    plain.set_boundary(BOUNDARY)
    plain.upload(POS)
    assert "not a tile context" in refused(bad, plain.tile_stats)
    assert L.sphx_tile_stats_record(plain.h, None, 0, 4, 1) == bad and L.sphx_tile_stats_frame(plain.h, 0.001, N) == bad
    assert L.sphx_tile_stats_read(plain.h, 0, 0, None, None) == bad
    assert plain.stats()[0]["count"] == N
    plain.close()
    m.close()


def test_solver_object_reaches_the_tiled_statistics():
    w = y.FluidParticleWorld()
    w.reset_fluid(1.0)
    s = y.DFSPHMultiSolver(w, [0, 0])
    t = y.TimeManager()
    assert "before the first sphx_multi_upload" in refused(_lib.ERR_NOT_READY, s.stats)  # (the solver uploads with its first step)
    refused(_lib.ERR_NOT_READY, s.stats_record, [EVERYTHING], 4, every=2)
    assert s.stats_status()["recording"] == 0
    s.simulation_step(w, t, sync_world=False)
    s.stats_record([EVERYTHING], 4, every=2)
    s.simulation_steps(w, t, 4, sync_world=True)
    rec, info = s.stats_frames()
    assert info["step"].tolist() == [2, 4] and s.stats_status()["frames"] == 2
    whole, tiles = s.stats([EVERYTHING], per_tile=True)
    assert whole.tobytes() == rec[1].tobytes() and tiles.shape == (2, 2)
    d = dict(pos=w.positions, vel=w.velocities, density=w.densities)
    check_all(whole, d, [EVERYTHING], "the solver object's tiles")
    single = y.DFSPHSolver(w)
    assert not single.L.sphx_solver_multi(single.h)
    single.close()
    s.close()


# ---- 9. one process per tile -------------------------------------------------------------------------------------------------------------------------
def test_rank_mode_every_rank_gets_the_bytes_of_the_in_process_run(tmp_path):
    """Two processes over gloo (the halo records) and the shared segment (the scalars, and with them the records of the statistics): both
    ranks hold identical bytes — whole fluid, per tile, and a recorded series — and these are the in-process devices=[0, 0] result of
    the same run."""
    steps, every = 24, 4
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1", "--master-port", "29547",
           os.path.join(HERE, "stats_multi_rank_worker.py"), str(tmp_path), str(steps), str(every)]
    p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    r = [np.load(tmp_path / f"rank{k}.npz") for k in range(2)]
    keys = ("whole0", "tiles0", "whole", "tiles", "frames", "info", "status")
    for k in keys:
        assert r[0][k].tobytes() == r[1][k].tobytes(), k
    m = make_multi(2)
    rects = [tuple(float(x) for x in v) for v in r[0]["rects"].tolist()]
    whole0, tiles0 = m.stats(rects, per_tile=True)
    m.stats_record(rects, 16, every=every)
    timer = y.TimeManager()
    m.steps(timer, steps)
    whole, tiles = m.stats(rects, per_tile=True)
    frames, info = m.stats_frames()
    assert frames.shape == (steps // every, 1 + len(rects)) and len(rects) == 3
    for k, v in (("whole0", whole0), ("tiles0", tiles0), ("whole", whole), ("tiles", tiles), ("frames", frames), ("info", info)):
        assert r[0][k].tobytes() == v.tobytes(), k
    assert r[0]["status"].tolist() == [m.stats_status()[k] for k in ("n_rects", "recording", "max_frames", "every", "frames", "dropped")]
    # and the truth: the ranks' owned particles together are the fluid
    d = {k: np.concatenate([r[0][k], r[1][k]]) for k in ("pos", "vel", "density")}
    check_all(r[0]["whole"].view(y.STATS_DTYPE).reshape(-1), d, rects, "two ranks")
    assert [int(c) for c in r[0]["tiles"].view(y.STATS_DTYPE).reshape(2, -1)[:, 0]["count"]] == [len(r[0]["pos"]), len(r[1]["pos"])]
    m.close()
