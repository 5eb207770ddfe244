"""Gauges and probes of a tiled run on the device (include/sphx.h, "gauges and probes of a tiled run"): sphx_multi_gauge_levels, the
sphx_multi_probe_* recorder and the fold of the ranks' parts.  The expected records never come from the calls under test: they are the
gauge rule (tests/gauge_reference.py) over the float32 restatement of sampling (tests/sample_reference.py) on the answering tile's own
downloads, or the single context in tiling-invariant mode.  Everything is compared as bits.  All scenes are the dam break of
tests/util.py at scale 1.0 (4 050 particles, every tile on device 0) with a halo of 10 cells and a re-partition every 4 steps, so that
ghosts, migration and moving cuts really happen.  The host side (intervals, the fold) is checked without a GPU in
tests/test_gauge_multi_host.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import gauge_multi_reference as gmr
import gauge_reference as gr
import sample_reference as sr
import test_gpu_sample_multi as sm
import yasph2d_amd as y
from yasph2d_amd import _lib

pytestmark = pytest.mark.gpu

F = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
POS, BOUNDARY, N, H = sm.POS, sm.BOUNDARY, sm.N, sm.H
KINDS = sm.KINDS
FIELDS = (("fraction", 0.5), ("density", 50.0))  # field, iso
TILINGS, TILING_IDS = sm.TILINGS, sm.TILING_IDS
bits, refused, new_multi = sm.bits, sm.refused, sm.new_multi
BED = [0.02, 0.75, 0.0071, 0.0, 120]  # dy == 0: the front along the bed
PROBES = np.array([[0.15, 0.75], [0.3, 0.9], [0.45, 1.2], [0.58, 1.55], [0.62, 0.76], [1.5, 0.7], [0.3, 2.5], [1e6, -1e6]], F)


def gauge_set(rects):
    """four columns through the fluid and above it; the bed gauge; an oblique ray with negative steps; a ray wholly outside the domain; a
    single sample, 65 and 129 samples (the trip boundaries of the reduce pass); and per cut one ray along its first and last owned cell
    row or column"""
    g = [[x, 0.6, 0.0, 0.013, 110] for x in (0.15, 0.3, 0.45, 0.58)]
    g += [BED, [0.75, 1.9, -0.006, -0.011, 110], [-300.0, -300.0, -0.5, -0.5, 9], [0.3, 0.8, 0.1, 0.1, 1], [0.2, 0.72, 0.002, 0.013, 65],
          [0.5, 0.65, -0.001, 0.009, 129]]
    cols, rows = set(), set()
    for x0, x1, y0, y1 in np.asarray(rects).tolist():
        cols |= {c for c in (x0, x1) if 0 < c < 65536}
        rows |= {c for c in (y0, y1) if 0 < c < 65536}
    for c in sorted(cols):
        g += [[float(sm.cell_centre(c - 1)), 0.6, 0.0, 0.013, 110], [float(sm.cell_centre(c)), 0.6, 0.0, 0.013, 110]]
    for c in sorted(rows):
        g += [[0.02, float(sm.cell_centre(c - 1)), 0.0071, 0.0, 120], [0.02, float(sm.cell_centre(c)), 0.0071, 0.0, 120]]
    return g


def reference_values(K, rects, states, pts, kind):
    owner = sm.owner_of(K, rects, pts)
    return sm.reference(K, states, owner, pts, kind), owner


def reference_parts(K, rects, gauges, values, iso):
    """[tiles, gauges] parts of the restatement: the brute-force intervals reduced over the reference values"""
    rows = gr.gauge_rows(gauges)
    out, at = np.zeros((len(rects), len(rows)), gmr.PART_DTYPE), 0
    for k, g in enumerate(rows):
        iv = gmr.intervals(g, K.gmin, K.cell_inv, np.asarray(rects).tolist())
        for t in range(len(rects)):
            out[t, k] = gmr.part_of(values[at:at + g[4]], int(iv[t, 0]), int(iv[t, 1]), iso)
        at += g[4]
    return out


def snapshot(m, what):
    rects, states = m.tile_rects(), sm.tile_states(m)
    gauges = gauge_set(rects)
    s = dict(what=what, rects=rects, states=states, gauges=gauges, pts=gr.all_points(gauges), calls={}, samples={})
    for kind in KINDS:
        s["samples"][kind] = m.sample(s["pts"], kind, tiles=True)
        for field, iso in FIELDS:
            s["calls"][kind, field] = m.gauges(gauges, iso, field, kind, values=True, tiles=True)
    s["again"] = m.gauges(gauges, 0.5, "fraction", KINDS[0], values=True, tiles=True)
    return s


@pytest.fixture(scope="module", params=TILINGS, ids=TILING_IDS)
def run40(request):
    world, strips = request.param
    m = new_multi(world, strips)
    m.upload(POS)
    snaps = [snapshot(m, "after the upload")]
    m.steps(y.TimeManager(), 40)
    snaps.append(snapshot(m, "after 40 steps"))
    if world > 1:
        assert m.info()["rebalances"] >= 1, m.info()
    yield world, m, sm.consts_of(m), snaps
    m.close()


# ---- 1. against the answering tile -------------------------------------------------------------------------------------------------------
def test_records_values_and_parts_equal_the_restatement_over_the_answering_tiles(run40):
    world, m, K, snaps = run40
    for s in snaps:
        what = "%d tiles, %s" % (world, s["what"])
        crossed = 0
        for kind in KINDS:
            ref, owner = reference_values(K, s["rects"], s["states"], s["pts"], kind)
            for field, iso in FIELDS:
                rec, values, parts = s["calls"][kind, field]
                assert np.array_equal(bits(values), bits(ref[field])), "%s kind %d %s: values differ from the restatement" % (what, kind, field)
                assert np.array_equal(bits(values), bits(s["samples"][kind][field])), "%s kind %d %s: values differ from multi.sample" % (what, kind, field)
                want = gr.reduce32(ref[field], s["gauges"], iso)
                assert gr.same_bytes(rec, want), "%s kind %d %s: records differ at gauges %s" % (
                    what, kind, field, [k for k in range(len(want)) if not gr.same_bytes(rec[k], want[k])])
                want_parts = reference_parts(K, s["rects"], s["gauges"], ref[field], iso)
                assert parts.shape == want_parts.shape and gr.same_bytes(parts, want_parts), "%s kind %d %s: parts differ" % (what, kind, field)
                assert gr.same_bytes(y.gauge_merge(parts, s["gauges"], iso), want)
                crossed += int(((parts["count"] > 0).sum(0) > 1).sum())
            if world > 1:
                assert len(np.unique(owner)) == world, what + ": the gauges do not reach every tile"
        rec = s["calls"][KINDS[0], "fraction"][0]
        assert (rec["inside"][:6] > 0).all() and (rec["last"][:4] < 109).all() and rec["inside"][6] == 0, what  # columns end dry, the outside ray is empty
        assert world == 1 or crossed > 0, what + ": no gauge crosses a cut"
        for a, b in zip(s["again"], s["calls"][KINDS[0], "fraction"]):  # two calls on one state: the same bytes
            assert gr.same_bytes(a, b)


# ---- 2. against a single context in tiling-invariant mode --------------------------------------------------------------------------------
@pytest.mark.parametrize("tiling", TILINGS, ids=TILING_IDS)
def test_tiling_invariant_mode_equals_the_single_context(tiling):
    world, strips = tiling
    fixed = (2, 2)
    m = new_multi(world, strips, params=y.default_params(fixed_iterations=fixed), halo=16, invariant=True)
    m.upload(POS)
    timer = y.TimeManager()
    for steps in (0, 40):
        if steps:
            m.steps(timer, steps)
        ctx = sm.single_context(steps, y.default_params(fixed_iterations=fixed))
        gauges = gauge_set(m.tile_rects())
        for kind in KINDS:
            for field, iso in FIELDS:
                got, want = m.gauges(gauges, iso, field, kind, values=True), ctx.gauges(gauges, iso, field, kind, values=True)
                assert gr.same_bytes(got[0], want[0]) and gr.same_bytes(got[1], want[1]), (world, steps, kind, field)
        ctx.close()
    m.close()


# ---- 3. the crossing on a cut ------------------------------------------------------------------------------------------------------------
def test_the_crossing_on_a_cut():
    """two fixed strips whose cut is chosen, with the numpy restatement over the uploaded state, so that for a bed gauge of one sample per
    cell column `last` and `last + 1` have different owners: f_last and f_next then live on different tiles"""
    params = y.default_params(fixed_iterations=(2, 2))
    K = sr.Constants(params)
    bed = [0.021, 0.75, float(H), 0.0, 60]  # (the step is the cell size: consecutive samples lie in consecutive cell columns)
    pts = gr.all_points([bed])
    state = dict(pos=POS, vel=np.zeros_like(POS), density=np.ones(N, F), boundary=BOUNDARY)
    cpu = gr.reduce32(sr.sample32(K, state, pts, sr.KERNEL_WENDLAND)["density"], [bed], 50.0)[0]
    last = int(cpu["last"])
    assert 0 < last < 58
    cells = sr.cells_of(K, pts)
    cut = int(cells[last + 1, 0])
    assert int(cells[last, 0]) == cut - 1
    m = new_multi(2, (0, [0, cut, 65536]), params=params, halo=16, rebalance_every=0, invariant=True)
    m.upload(POS)
    ctx = sm.single_context(0, params)
    rects = m.tile_rects()
    assert rects.tolist() == [[0, cut, 0, 65536], [cut, 65536, 0, 65536]]
    gauges = [bed] + gauge_set(rects)
    for kind in KINDS:
        for field, iso in FIELDS:
            rec, parts = m.gauges(gauges, iso, field, kind, tiles=True)
            want = ctx.gauges(gauges, iso, field, kind)
            assert gr.same_bytes(rec, want), (kind, field, rec[0], want[0])
            if (kind, field) == (KINDS[0], "density"):
                # the precondition: the owner of `last` ends there, the other tile begins at last + 1 and holds f_next in its f_lo alone
                assert int(rec["last"][0]) == last and sm.owner_of(K, rects, pts[last:last + 2]).tolist() == [0, 1]
                assert int(parts[0, 0]["lo"] + parts[0, 0]["count"]) == last + 1 and int(parts[1, 0]["lo"]) == last + 1
                assert bits(parts[0, 0]["f_next"]) == gr.QNAN and bits(parts[1, 0]["f_lo"]) == bits(rec["f_next"][0]) and parts[1, 0]["inside"] == 0
    ctx.close()
    m.close()


# ---- 4. the recorder ---------------------------------------------------------------------------------------------------------------------
def lopsided_multi(world):
    """a layout that starts far from balance (a fifth of the fluid's columns on the left), so that the first re-partition, behind step 4,
    moves the cuts for certain"""
    m = sm.MultiSolver(y.default_params(), devices=[0] * world, halo=10, rebalance_every=4)
    if world == 2:
        m.set_strips(0, [0, 5010, 65536])
    else:
        m.set_grid([0, 5010, 65536], [[0, 5040, 65536], [0, 5036, 65536]])
    m.set_boundary(BOUNDARY)
    return m


@pytest.mark.parametrize("world", [2, 4], ids=["2 strips", "2x2"])
def test_recorded_frames_equal_one_shot_calls_of_a_twin_run(world):
    """frames taken inside steps(k) against one-shot calls made behind the same steps of a twin run; `every`, `dropped`, a sub-range
    read, a re-partition between frames, and a recording started before the upload"""
    every, max_frames, steps = 2, 6, 16
    rec_m = lopsided_multi(world)
    gauges = gauge_set([[0, 5017, 0, 65536]]) + [[float(sm.cell_centre(c)), 0.6, 0.0, 0.013, 110] for c in range(5008, 5030, 3)]
    rec_m.probe_record(PROBES, gauges, max_frames, every, iso=0.5, field="fraction", kernel=y.KERNEL_WENDLAND_C2)  # before the upload
    st = rec_m.probe_status()
    assert st == dict(m_points=len(PROBES), n_gauges=len(gauges), recording=1, max_frames=max_frames, every=every, frames=0, dropped=0)
    rec_m.upload(POS)
    rec_m.steps(y.TimeManager(), steps)
    st = rec_m.probe_status()
    assert st["frames"] == max_frames and st["dropped"] == steps // every - max_frames and st["recording"] == 1
    assert rec_m.info()["rebalances"] >= 1
    frames = rec_m.probe_frames(tiles=True)
    assert frames["info"]["step"].tolist() == [every * (k + 1) for k in range(max_frames)] and (frames["info"]["n"] == N).all()
    twin = lopsided_multi(world)
    twin.upload(POS)
    timer = y.TimeManager()
    rects_seen = set()
    for k in range(1, every * max_frames + 1):
        stats = twin.step(timer)
        if k % every:
            continue
        f = k // every - 1
        assert frames["info"]["dt"][f] == F(stats["dt"])
        want = twin.gauges(gauges, 0.5, "fraction", y.KERNEL_WENDLAND_C2)
        assert gr.same_bytes(frames["gauges"][f], want), "frame %d: gauges %s differ" % (f, [g for g in range(len(want)) if not gr.same_bytes(frames["gauges"][f][g], want[g])])
        pts = twin.sample(PROBES, y.KERNEL_WENDLAND_C2, tiles=True)
        got = frames["points"][f]
        for name in ("density", "fraction", "velocity", "count"):
            assert np.array_equal(bits(got[name]), bits(pts[name])), (f, name)
        assert not got["reserved"].any() and np.array_equal(frames["point_tile"][f], pts["tile"])
        rects_seen.add(twin.tile_rects().tobytes())
    assert len(rects_seen) > 1, "the cuts did not move between the frames"
    assert (frames["gauges"]["inside"][:, :4] > 0).all() and len({frames["gauges"][f].tobytes() for f in range(max_frames)}) == max_frames
    # a sub-range, and the ranges beyond the frames
    part = rec_m.probe_frames(first=2, count=3)
    for name in ("points", "gauges", "info"):
        assert gr.same_bytes(part[name], frames[name][2:5]), name
    assert "beyond the frames" in refused(_lib.ERR_INVALID_ARGUMENT, rec_m.probe_frames, first=4, count=3)
    assert len(rec_m.probe_frames(first=6)["info"]) == 0
    # a new recording discards the old; max_frames == 0 stops and frees
    rec_m.probe_record(PROBES[:2], None, 3, 1)
    assert rec_m.probe_status() == dict(m_points=2, n_gauges=0, recording=1, max_frames=3, every=1, frames=0, dropped=0)
    rec_m.steps(timer, 1)
    one = rec_m.probe_frames()
    assert one["gauges"].shape == (1, 0) and one["points"].shape == (1, 2) and one["info"]["step"].tolist() == [1]
    pts = rec_m.sample(PROBES[:2], y.KERNEL_WENDLAND_C2)  # (the last frame is the state the multi is in)
    assert np.array_equal(bits(one["points"][0]["density"]), bits(pts["density"])) and np.array_equal(one["points"][0]["count"], pts["count"])
    rec_m.probe_record(None, None, 0)
    assert rec_m.probe_status()["recording"] == 0 and rec_m.probe_status()["frames"] == 0
    twin.close()
    rec_m.close()


# ---- 5. no trace in the run --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 4], ids=["2 strips", "2x2"])
def test_recording_and_calls_leave_no_trace_in_the_run(world):
    gauges = gauge_set([[0, 5017, 0, 65536]])
    runs = []
    for gauging in (False, True):
        m = new_multi(world)
        m.upload(POS)
        if gauging:
            m.probe_record(PROBES, gauges, 64, 3)
        timer = y.TimeManager()
        stats = []
        for _ in range(40):
            stats.append(m.step(timer))
            if gauging:
                m.gauges(gauges, values=True)
                m.gauges(gauges[:3], 50.0, "density", y.KERNEL_SPIKY)
        d = m.download()
        order = np.argsort(d["ids"], kind="stable")
        digest = m.state_digest()
        m.step_begin(timer.simulation_step())
        runs.append(dict(stats=stats, d={k: v[order] for k, v in d.items()}, digest=digest, exchanges=m.info()["exchanges"], rebalances=m.info()["rebalances"]))
        if gauging:
            assert m.probe_status()["frames"] == 13
        m.close()
    a, b = runs
    for k in range(40):
        assert set(sm.STEP_FIELDS) - {"reserved"} <= set(a["stats"][k]) and a["stats"][k] == b["stats"][k], (k, a["stats"][k], b["stats"][k])
    for f in a["d"]:
        assert np.array_equal(bits(a["d"][f]), bits(b["d"][f])), f
    assert a["digest"] == b["digest"] and a["exchanges"] == b["exchanges"] and a["rebalances"] == b["rebalances"] >= 1


# ---- 6. a spent ghost band ---------------------------------------------------------------------------------------------------------------
def test_a_spent_ghost_band_is_refreshed_by_the_call():
    """the set-up of test_a_spent_ghost_band_is_refreshed_by_the_query: a fixed halo of 7 cells, 2 density and 3 divergence iterations"""
    fixed = (2, 3)
    m = new_multi(2, None, params=y.default_params(fixed_iterations=fixed), halo=7, fixed_halo=True, invariant=True)
    m.upload(POS)
    timer = y.TimeManager()
    m.steps(timer, 6)
    rings = m.ghost_rings()
    assert rings["valid"] < 1, rings  # the precondition of this test: the band is spent at the call
    ctx = sm.single_context(6, y.default_params(fixed_iterations=fixed))
    gauges = gauge_set(m.tile_rects())
    before = m.info()["exchanges"]
    got = m.gauges(gauges, values=True)
    assert m.info()["exchanges"] == before + 1  # exactly one exchange
    after = m.ghost_rings()
    assert after["valid"] == 7 and after["avalid"] == 6, after
    want = ctx.gauges(gauges, values=True)
    assert gr.same_bytes(got[0], want[0]) and gr.same_bytes(got[1], want[1])
    assert gr.same_bytes(m.gauges(gauges, 50.0, "density"), ctx.gauges(gauges, 50.0, "density"))
    assert m.info()["exchanges"] == before + 1  # (the second call found a full band)
    m.step_begin(timer.simulation_step())
    assert m.info()["exchanges"] == before + 1  # ... and so does the step: the exchange it owed has happened
    m.step_finish(F(0.0005))
    # a recorded frame pulls the same exchange forward: as many exchanges as the run without, and the last frame is the one-shot call
    counts = []
    for recording in (False, True):
        r = new_multi(2, None, params=y.default_params(fixed_iterations=fixed), halo=7, fixed_halo=True, invariant=True)
        r.upload(POS)
        if recording:
            r.probe_record(PROBES, gauges, 8, 1)
        t = y.TimeManager()
        r.steps(t, 6)
        if recording:
            assert r.ghost_rings()["valid"] == 7  # the frame of step 6 has refreshed the band
            fr = r.probe_frames()
            assert len(fr["info"]) == 6 and gr.same_bytes(fr["gauges"][5], want[0])
        r.step_begin(t.simulation_step())
        counts.append(r.info()["exchanges"])
        r.close()
    assert counts[0] == counts[1], counts
    ctx.close()
    m.close()


# ---- 7. refusals and no-ops --------------------------------------------------------------------------------------------------------------
def test_refusals_and_no_ops():
    bad, not_ready = _lib.ERR_INVALID_ARGUMENT, _lib.ERR_NOT_READY
    m = new_multi(2)
    L = m.L
    good = y._gauge_array([[0.3, 0.6, 0.0, 0.013, 40]])
    rec = np.zeros(4, y.GAUGE_REC_DTYPE)

    def call(g=good, n=None, kind=0, field=0, iso=0.5, flags=0, out=rec):
        rc = L.sphx_multi_gauge_levels(m.h, g.ctypes.data if g is not None and len(g) else None, (len(g) if g is not None else 0) if n is None else n, kind,
                                       field, iso, flags, out.ctypes.data if out is not None else None, None, None)
        return rc, L.sphx_multi_last_error(m.h).decode()

    def one(**kw):
        g = good.copy()
        for k, v in kw.items():
            g[k] = v
        return g

    # the argument errors of the single call (they name the argument), before the first upload too
    for kw, word in ((dict(out=None), "out is NULL"), (dict(g=None, n=1), "gauges is NULL"), (dict(kind=3), "kernel_kind"), (dict(field=2), "field"),
                     (dict(flags=1), "flags"), (dict(iso=float("nan")), "iso"), (dict(g=one(n=0)), "n == 0"), (dict(g=one(n=2 ** 20 + 1)), "2^20"),
                     (dict(g=one(x0=np.nan)), "non-finite"), (dict(g=one(dy=np.inf)), "non-finite"),
                     (dict(g=np.repeat(one(n=2 ** 20), 17), out=np.zeros(17, y.GAUGE_REC_DTYPE)), "2^24"),
                     (dict(g=np.repeat(good, _lib.GAUGE_MAX + 1), out=np.zeros(_lib.GAUGE_MAX + 1, y.GAUGE_REC_DTYPE)), "SPHX_GAUGE_MAX")):
        rc, msg = call(**kw)
        assert rc == bad and word in msg and msg.startswith("sphx_multi_gauge_levels: "), (kw.keys(), msg)
    assert call(g=None)[0] == 0 and call(n=0)[0] == 0  # n_gauges == 0 succeeds, whatever the state
    rc, msg = call()
    assert rc == not_ready and "upload" in msg  # before the first upload
    for kw, word in ((dict(every=0), "every"), (dict(points=np.zeros((0, 2), F), gauges=None), "nothing to record")):
        args = dict(points=PROBES, gauges=good, max_frames=4, every=1)
        args.update(kw)
        assert word in refused(bad, m.probe_record, **args)
    assert "64 MiB" in refused(_lib.ERR_CAPACITY, m.probe_record, PROBES, good, max_frames=2 ** 20)
    assert "beyond the frames" in refused(bad, m.probe_frames, first=0, count=1)
    assert m.probe_status() == dict(m_points=0, n_gauges=0, recording=0, max_frames=0, every=0, frames=0, dropped=0)
    m.upload(POS)
    assert call()[0] == 0 and rec["inside"][0] > 0
    # inside an open step
    timer = y.TimeManager()
    m.step_begin(timer.simulation_step())
    rc, msg = call()
    assert rc == not_ready and "step" in msg
    assert "step" in refused(not_ready, m.probe_record, PROBES, good, 4)
    assert "step" in refused(not_ready, m.probe_frames)
    m.step_finish(F(0.001))
    assert call()[0] == 0
    # the plain calls still refuse a tile, with their present message; the seam refuses a plain context
    t = m.tile_context(0)
    for fn, args in ((t.gauges, (good,)), (t.probe_record, (PROBES, good, 4)), (t.probe_frames, ())):
        assert "not available on a tile context" in refused(bad, fn, *args)
    ctx = y.SphxContext()
    assert L.sphx_tile_gauge_levels(ctx.h, good.ctypes.data, 1, 0, 0, 0.5) == bad and "not a tile context" in L.sphx_last_error(ctx.h).decode()
    assert L.sphx_tile_probe_record(ctx.h, None, 0, good.ctypes.data, 1, 0, 0, 0.5, 4, 1) == bad
    assert L.sphx_tile_probe_frame(ctx.h, 0.001, 0) == bad and L.sphx_tile_probe_due(ctx.h) == 0
    ctx.close()
    m.close()


def test_solver_object_reaches_the_tiled_gauges():
    w = y.FluidParticleWorld()
    w.reset_fluid(1.0)
    s = y.DFSPHMultiSolver(w, [0, 0])
    t = y.TimeManager()
    gauges = gauge_set([[0, 5017, 0, 65536]])
    s.probe_record(PROBES, gauges, 4, 1)  # (the solver uploads with its first step: the recording waits for it)
    s.simulation_steps(w, t, 5, sync_world=False)
    assert s.probe_status()["frames"] == 4 and s.probe_status()["dropped"] == 1
    rec, values = s.gauges(gauges, values=True)
    assert gr.same_bytes(rec, y.gauge_reduce(values, gauges, 0.5)) and gr.same_bytes(values, s.sample(gr.all_points(gauges), fields="fraction")["fraction"])
    fr = s.probe_frames()
    assert fr["gauges"].shape == (4, len(gauges)) and (fr["gauges"]["inside"][:, :4] > 0).all()
    s.close()


# ---- 8. one process per tile -------------------------------------------------------------------------------------------------------------
def test_rank_mode_parts_fold_to_the_in_process_run(tmp_path):
    """Two fresh processes over gloo (the halo records) and the shared segment (the scalars), both on device 0.  Each rank returns its
    parts; folded with gauge_merge they are the records of the in-process devices=[0, 0] run, one-shot and recorded."""
    steps = 12
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1", "--master-port", "29571",
           os.path.join(HERE, "gauge_multi_rank_worker.py"), str(tmp_path), str(steps)]
    p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert p.returncode == 0, p.stderr.decode()[-3000:]
    r = [np.load(tmp_path / f"rank{k}.npz") for k in range(2)]
    gauges = r[0]["gauges"]
    assert gr.same_bytes(gauges, r[1]["gauges"])
    m = new_multi(2)
    m.probe_record(PROBES, gauges, 8, 3)
    m.upload(POS)
    m.steps(y.TimeManager(), steps)
    want, parts = m.gauges(gauges, tiles=True)
    for k in range(2):
        assert r[k]["refused_without_parts"] == _lib.ERR_INVALID_ARGUMENT
        assert gr.same_bytes(r[k]["parts"].reshape(-1), parts[k]), k  # a rank's part is that tile's part
    assert ((parts["count"] > 0).sum(0) > 1).any()  # some gauge does cross the ranks
    assert gr.same_bytes(y.gauge_merge([r[0]["parts"], r[1]["parts"]], gauges, 0.5), want)
    with pytest.raises(y.SphxError):
        y.gauge_merge([r[0]["parts"]], gauges, 0.5)  # one rank alone leaves gaps
    frames = m.probe_frames(tiles=True)
    assert len(frames["info"]) == 4
    for f in range(4):
        assert gr.same_bytes(y.gauge_merge([r[0]["frame_parts"][f], r[1]["frame_parts"][f]], gauges, 0.5), frames["gauges"][f]), f
        tiles = np.stack([r[k]["frame_point_tile"][f] for k in range(2)])
        assert np.array_equal(np.where(tiles[0] >= 0, tiles[0], tiles[1]), frames["point_tile"][f])
        for k in range(2):
            mine = tiles[k] == k
            assert gr.same_bytes(r[k]["frame_points"][f][mine], frames["points"][f][mine]) and not r[k]["frame_points"][f][~mine].view(np.uint8).any()
    m.close()
