"""Fluid statistics on the device (include/sphx.h, "fluid statistics"): sphx_fluid_stats and the recorder sphx_stats_record / _read against
tests/stats_reference.py — the terms in float64 as the header writes them, math.fsum for the exact sums.  Counts, extremes and
max_speed_sq are compared bit for bit, every sum against the stated bound n * 2^-52 * fsum(|t|).  The layouts, the exports, the NULL
refusals and the reference itself are checked without a GPU in tests/test_stats_host.py."""
import json
import os
import subprocess

import numpy as np
import pytest

import stats_reference as ref
import yasph2d_amd as y
from util import uniform_points
from yasph2d_amd import _lib

pytestmark = pytest.mark.gpu

F = np.float32
INF = float("inf")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "dam_break_4050.npz"))
POS, BOUNDARY = GOLD["in_pos"], GOLD["in_boundary"]
DIAM = F(0.01)
HARNESS = os.path.join(os.path.dirname(os.path.abspath(y.__file__)), "sphx_harness")
EVERYTHING = (-INF, -INF, INF, INF)


def refused(code, fn, *args, **kw):
    with pytest.raises(y.SphxError) as e:
        fn(*args, **kw)
    assert e.value.code == code, str(e.value)
    return str(e.value)


def dfsph_step(ctx, timer, dts=None):
    vmax = ctx.step_begin(timer.simulation_step(), timer.law(DIAM))
    dt = y.duration_as_secs_f32(timer.update_simulation_step(DIAM, vmax))
    if dts is not None:
        dts.append(dt)
    return ctx.step_finish(dt)


def wcsph_step(ctx, timer, dts=None):
    vmax = ctx.wcsph_step_begin(timer.simulation_step())
    dt = y.duration_as_secs_f32(timer.update_simulation_step(DIAM, vmax))
    if dts is not None:
        dts.append(dt)
    return ctx.wcsph_step_finish(dt)


def dam_context():
    ctx = y.SphxContext()
    ctx.set_boundary(BOUNDARY)
    ctx.upload(POS)
    return ctx


def check_all(got, d, rects, density_valid, what):
    """every record of one call against the reference; -> the reference records.  Each figure of a sum is printed before it is judged."""
    want = ref.stats(d, rects, density_valid)
    assert got.dtype == y.STATS_DTYPE and got.shape == (1 + len(rects),)
    for r, (g, w) in enumerate(zip(got, want)):
        for k in ref.SUMS:
            gs, ws, ab = np.atleast_1d(g[k]), np.atleast_1d(w[k]), np.atleast_1d(w["abs_" + k])
            for j in range(len(gs)):
                print("%s record %d %s[%d]: device %.17g exact %.17g |diff| %.3g bound %.3g" % (
                    what, r, k, j, gs[j], ws[j], abs(float(gs[j]) - float(ws[j])), w["n_" + k] * ref.U * ab[j]))
        ref.check(g, w, "%s, record %d" % (what, r))
    return want


# ---- 1. sizes ---------------------------------------------------------------------------------------------------------------------------------
# stage 1 takes 1 024 particles per workgroup (up to 2 048 workgroups), stage 2 folds 256 partial records per pass: 300 000 particles are
# 293 stage-1 workgroups — many chunks, a ragged last one, and more partials than one stage-2 pass takes
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 300000])
def test_sizes_against_the_reference(n):
    pos = (uniform_points(n, 10000.0, 100 + n) + F(0.3)).astype(F) if n else np.zeros((0, 2), F)
    vel = np.random.default_rng(n).standard_normal((n, 2)).astype(F)
    side = float(np.sqrt(n / 10000.0)) if n else 1.0
    rects = [(0.3 + 0.25 * side, 0.3 + 0.1 * side, 0.3 + 0.8 * side, 0.3 + 0.6 * side), EVERYTHING]
    ctx = y.SphxContext()
    ctx.upload(pos, vel)
    got = ctx.stats(rects)
    assert (got["density_valid"] == 0).all() and (got["reserved"] == 0).all()
    d = ctx.download()
    assert np.array_equal(d["pos"], pos)  # (an upload keeps the order)
    want = check_all(got, d, rects, False, "n = %d after the upload" % n)
    assert got[0]["count"] == n == got[2]["count"] and (n < 64 or 0 < got[1]["count"] < n)
    ctx.update_neighborhood()
    ctx.update_densities()
    try:  # density_valid is "the state in which sphx_sample_* succeeds" (a build over zero particles leaves nothing to sample)
        ctx.sample(np.array([[0.5, 0.5]], F), fields=("density",))
        valid = True
    except y.SphxError:
        valid = False
    assert valid or n == 0
    got = ctx.stats(rects)
    assert (got["density_valid"] == int(valid)).all()
    d = ctx.download()
    want = check_all(got, d, rects, valid, "n = %d with densities" % n)
    if n:
        assert got[0]["density_count"] == n and got[0]["min_density"] > 0 and want[0]["sum_density"] > 0
        assert got[0]["min_density"] == d["density"].min() and got[0]["max_density"] == d["density"].max()
    assert ctx.stats().shape == (1,) and ctx.stats().tobytes() == got[:1].tobytes()  # (a record does not depend on the others)


# ---- 2. rectangles ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dam5():
    """dam_break_4050 after 5 adaptive DFSPH steps and its download: shared, never stepped again"""
    ctx, timer = dam_context(), y.TimeManager()
    for _ in range(5):
        dfsph_step(ctx, timer)
    return ctx, ctx.download()


def dam_rects(d):
    p = d["pos"]
    xs, ys = np.sort(p[:, 0]), np.sort(p[:, 1])
    return [(0.9, 0.0, 0.1, 2.0),                      # inverted: empty
            EVERYTHING,                                # equals record 0
            (0.0, 0.6, 0.35, 1.2), (0.2, 0.9, 0.6, 1.5),  # two that overlap
            (float(xs[500]), float(ys[700]), float(xs[3000]), float(ys[3500])),  # every edge passes exactly through particle coordinates
            (-INF, 0.95, 0.4, INF),                    # half infinite
            (5.0, 5.0, 6.0, 6.0),                      # no particle
            (0.31, 1.01, 0.33, 1.03)]                  # a small probe


def test_eight_rectangles_on_the_dam_break(dam5):
    ctx, d = dam5
    rects = dam_rects(d)
    assert len(rects) == _lib.STATS_MAX_RECTS
    got = ctx.stats(rects)
    want = check_all(got, d, rects, True, "dam break")
    counts = got["count"].tolist()
    assert counts[0] == 4050 == counts[2] and counts[1] == 0 == counts[7] and 0 < counts[8] < 50 and (got["nonfinite"] == 0).all()
    assert all(0 < c < 4050 for c in (counts[3], counts[4], counts[5], counts[6]))
    inside = ref.inside(d["pos"], rects[2]) & ref.inside(d["pos"], rects[3])
    assert inside.any()  # (the overlap holds particles: both records count them)
    e = rects[4]
    on_edge = [(d["pos"][:, 0] == F(e[0])).any(), (d["pos"][:, 1] == F(e[1])).any(), (d["pos"][:, 0] == F(e[2])).any(), (d["pos"][:, 1] == F(e[3])).any()]
    assert all(on_edge)
    # the all-covering rectangle against record 0: another order of addition, the same exact members
    for k in ref.EXACT:
        assert ref.bits(got[2][k]) == ref.bits(got[0][k]), k
    for k in ref.SUMS:
        a, b, ab = np.atleast_1d(got[2][k]), np.atleast_1d(got[0][k]), np.atleast_1d(want[0]["abs_" + k])
        for j in range(len(a)):
            assert abs(float(a[j]) - float(b[j])) <= 2 * want[0]["n_" + k] * ref.U * ab[j], (k, j, a[j], b[j])
    # fewer rectangles: the same records
    assert ctx.stats(rects[3:5]).tobytes() == got[[0, 4, 5]].tobytes()


# ---- 3. non-finite values -----------------------------------------------------------------------------------------------------------------------
def test_nonfinite_particles_are_counted_and_summed_nowhere():
    """NaN and +-inf velocities — and non-finite positions, uploaded the way tests/test_gpu_render.py uploads them — without a step"""
    pos = POS.copy()
    vel = np.random.default_rng(3).standard_normal(pos.shape).astype(F)
    clean_vel = vel.copy()
    vel[10] = (np.nan, 1.0)
    vel[11] = (2.0, np.inf)
    vel[12] = (-np.inf, np.nan)
    vel[2000::500] = (np.nan, np.nan)
    bad_pos = [(np.nan, 0.5), (0.5, np.nan), (np.inf, 0.5), (0.5, -np.inf), (-np.inf, np.inf), (np.nan, np.nan)]
    where = np.arange(100, 100 + 97 * len(bad_pos), 97)
    ctx = y.SphxContext()
    ctx.set_boundary(BOUNDARY)
    try:
        p = pos.copy()
        p[where] = np.array(bad_pos, F)
        ctx.upload(p, vel)
        pos = p
    except y.SphxError:  # sphx_upload does not take non-finite positions: the velocities remain
        ctx.upload(pos, vel)
    rects = [EVERYTHING, (0.0, 0.6, 0.3, 1.0), (0.3, -INF, INF, INF)]
    got = ctx.stats(rects)
    d = ctx.download()
    check_all(got, d, rects, False, "non-finite")
    fin = np.isfinite(d["pos"]).all(axis=1) & np.isfinite(d["vel"]).all(axis=1)
    assert got[0]["nonfinite"] == (~fin).sum() >= 3 + len(vel[2000::500]) and got[0]["count"] == fin.sum()
    # a NaN coordinate is in no rectangle, an infinite one where the comparisons put it
    assert got[1]["nonfinite"] == (~fin & ref.inside(d["pos"], EVERYTHING)).sum() and got[1]["count"] == got[0]["count"]
    assert got[3]["nonfinite"] == (~fin & ref.inside(d["pos"], rects[2])).sum()
    # the sums are those of the finite particles alone
    only = ctx.stats()
    ctx2 = y.SphxContext()
    ctx2.set_boundary(BOUNDARY)
    ctx2.upload(d["pos"][fin], d["vel"][fin])
    alone = ctx2.stats()[0]
    w = ref.stats((d["pos"][fin], d["vel"][fin], np.zeros(fin.sum(), F)), (), False)[0]
    ref.check(alone, w, "the finite particles alone")
    for k in ("min_pos", "max_pos", "max_speed_sq", "count"):
        assert ref.bits(alone[k]) == ref.bits(only[0][k]), k
    assert np.array_equal(clean_vel[fin], d["vel"][fin])


# ---- 4. determinism ---------------------------------------------------------------------------------------------------------------------------
def test_two_calls_and_both_paths_return_the_same_bytes(dam5):
    import torch

    ctx, d = dam5
    rects = dam_rects(d)
    a, b = ctx.stats(rects), ctx.stats(rects)
    assert a.tobytes() == b.tobytes()
    out = torch.full((9 * 128,), 0xFF, dtype=torch.uint8, device="cuda")
    assert ctx.stats(rects, out=out) is out
    assert out.cpu().numpy().tobytes() == a.tobytes()
    out2 = torch.full((128,), 0xFF, dtype=torch.uint8, device="cuda")
    ctx.stats(out=out2)
    assert out2.cpu().numpy().tobytes() == a[:1].tobytes() == ctx.stats().tobytes()
    big = ctx_300k()
    r = [(0.5, 0.5, 3.0, 2.0), EVERYTHING]
    first = big.stats(r)
    out3 = torch.full((3 * 128,), 0xFF, dtype=torch.uint8, device="cuda")
    big.stats(r, out=out3)
    assert first.tobytes() == big.stats(r).tobytes() == out3.cpu().numpy().tobytes()
    with pytest.raises(ValueError):
        ctx.stats(rects, out=out2)


def ctx_300k():
    n = 300000
    ctx = y.SphxContext()
    ctx.upload((uniform_points(n, 10000.0, 7) + F(0.3)).astype(F), np.random.default_rng(8).standard_normal((n, 2)).astype(F))
    return ctx


# ---- 5. the recorder --------------------------------------------------------------------------------------------------------------------------
def test_recorder_against_a_twin_context():
    rects = [(0.0, 0.6, 0.35, 1.2), EVERYTHING]
    a, ta, b, tb = dam_context(), y.TimeManager(), dam_context(), y.TimeManager()
    assert a.stats_status() == dict(n_rects=0, recording=0, max_frames=0, every=0, frames=0, dropped=0)
    a.stats_record(rects, 3, every=3)
    assert a.stats_status() == dict(n_rects=2, recording=1, max_frames=3, every=3, frames=0, dropped=0)
    dts, want = [], []
    for s in range(12):
        sa, sb = dfsph_step(a, ta, dts), dfsph_step(b, tb)
        assert sa == sb
        want.append(b.stats(rects))
    assert a.stats_status() == dict(n_rects=2, recording=1, max_frames=3, every=3, frames=3, dropped=1)
    rec, info = a.stats_frames()
    assert rec.shape == (3, 3) and rec.dtype == y.STATS_DTYPE and info.dtype == y.STATS_FRAME_DTYPE
    assert info["step"].tolist() == [3, 6, 9] and info["n"].tolist() == [4050] * 3
    assert info["dt"].tobytes() == np.array([dts[2], dts[5], dts[8]], F).tobytes()
    for f, s in enumerate((2, 5, 8)):
        assert rec[f].tobytes() == want[s].tobytes(), "frame %d against stats() after step %d of the twin" % (f, s + 1)
    assert not np.array_equal(rec[0]["sum_pos"], rec[2]["sum_pos"]) and (rec["density_valid"] == 1).all()
    check_all(rec[2], b_download_after(9), rects, True, "frame 2")
    one, one_info = a.stats_frames(1, 1)
    assert one.tobytes() == rec[1:2].tobytes() and one_info.tobytes() == info[1:2].tobytes()
    assert a.stats_frames(3, 0)[0].shape == (0, 3)
    assert "first_frame + n_frames" in refused(_lib.ERR_INVALID_ARGUMENT, a.stats_frames, 3, 1)
    refused(_lib.ERR_INVALID_ARGUMENT, a.stats_frames, 0, 4)
    refused(_lib.ERR_INVALID_ARGUMENT, a.stats_frames, 0xFFFFFFFF, 2)
    # a failed step takes no frame and does not count; a new record discards the old one
    a.stats_record((), 4, every=2)
    assert a.stats_status() == dict(n_rects=0, recording=1, max_frames=4, every=2, frames=0, dropped=0)
    dfsph_step(a, ta)
    a.step_begin(ta.simulation_step())
    refused(_lib.ERR_INVALID_ARGUMENT, a.step_finish, F(-1.0))
    assert a.stats_status()["frames"] == 0
    dts = []
    dfsph_step(a, ta, dts)
    rec, info = a.stats_frames()
    assert rec.shape == (1, 1) and info["step"].tolist() == [2] and info["dt"][0] == F(dts[0])
    assert rec[0].tobytes() == a.stats().tobytes()
    a.stats_record((), 0)  # stop and free
    assert a.stats_status() == dict(n_rects=0, recording=0, max_frames=0, every=0, frames=0, dropped=0)
    dfsph_step(a, ta)
    assert a.stats_status()["frames"] == 0
    refused(_lib.ERR_INVALID_ARGUMENT, a.stats_frames, 0, 1)


def b_download_after(steps):
    """the download of a fresh dam break after `steps` adaptive DFSPH steps"""
    ctx, timer = dam_context(), y.TimeManager()
    for _ in range(steps):
        dfsph_step(ctx, timer)
    return ctx.download()


def test_recorder_with_wcsph_and_across_append_and_remove():
    rects = [(0.0, 0.6, 0.35, 1.2)]
    ctx, timer = dam_context(), y.TimeManager(cfl_factor=0.2)
    ctx.stats_record(rects, 8)
    want, dts = [], []
    for _ in range(3):
        wcsph_step(ctx, timer, dts)
        want.append(ctx.stats(rects))
    rec, info = ctx.stats_frames()
    assert info["step"].tolist() == [1, 2, 3] and info["dt"].tobytes() == np.array(dts, F).tobytes()
    assert rec.tobytes() == np.stack(want).tobytes() and (rec["density_valid"] == 1).all()
    check_all(rec[2], ctx.download(), rects, True, "WCSPH frame 2")
    # the recording belongs to the context: edits leave it alone, the frames see the new particle set
    ctx, timer = dam_context(), y.TimeManager()
    ctx.stats_record(rects, 8)
    dfsph_step(ctx, timer)
    extra = (np.array([1.2, 1.0], F) + np.stack(np.meshgrid(np.arange(20), np.arange(20)), -1).reshape(-1, 2).astype(F) * F(0.0111)).astype(F)
    ctx.append(extra, np.full_like(extra, -1.0))
    dfsph_step(ctx, timer)
    removed = ctx.remove((0.2, 0.4, 0.7, 0.9))
    assert removed > 0
    dfsph_step(ctx, timer)
    st = ctx.stats_status()
    assert (st["recording"], st["frames"], st["dropped"]) == (1, 3, 0)
    rec, info = ctx.stats_frames()
    assert info["n"].tolist() == [4050, 4450, 4450 - removed] and rec[:, 0]["count"].tolist() == info["n"].tolist()
    assert rec[2].tobytes() == ctx.stats(rects).tobytes()
    ctx.upload(POS[:1000])  # ... an upload and a state load too
    ctx.load_state(ctx.save_state())
    assert ctx.stats_status()["frames"] == 3 and ctx.stats_frames()[0].tobytes() == rec.tobytes()


# ---- 6. no side effects -----------------------------------------------------------------------------------------------------------------------
def test_no_side_effects():
    import torch

    rects = [(0.0, 0.6, 0.35, 1.2), EVERYTHING, (0.9, 0.0, 0.1, 2.0)]
    a, ta, b, tb = dam_context(), y.TimeManager(), dam_context(), y.TimeManager()
    a.stats(rects)
    a.stats_record(rects, 6, every=2)
    out = torch.zeros(4 * 128, dtype=torch.uint8, device="cuda")
    for s in range(10):
        sa, sb = dfsph_step(a, ta), dfsph_step(b, tb)
        assert sa == sb, "step %d" % s
        assert a.last_flags() == b.last_flags()
        assert a.state_digest() == b.state_digest(), "step %d" % s
        a.stats(rects)
        a.stats(rects, out=out)
        a.stats()
    assert a.stats_status()["frames"] == 5 and len(a.state_digest()) == 9
    assert ta.simulation_step_ns() == tb.simulation_step_ns() and ta.total_simulated_ns == tb.total_simulated_ns
    assert a.stats_frames()[0][-1].tobytes() == b.stats(rects).tobytes()


# ---- 7. state rules and argument errors -------------------------------------------------------------------------------------------------------
def test_state_rules_and_argument_errors():
    ctx = y.SphxContext()
    L, h, bad = ctx.L, ctx.h, _lib.ERR_INVALID_ARGUMENT
    # before any upload: N = 0, empty records
    got = ctx.stats([EVERYTHING])
    want = ref.stats((np.zeros((0, 2), F), np.zeros((0, 2), F), np.zeros(0, F)), [EVERYTHING], False)
    for g, w in zip(got, want):
        ref.check(g, w, "before any upload")
    assert got["min_pos"].tolist() == [[INF, INF]] * 2 and got["max_density"].tolist() == [-INF] * 2 and got["max_speed_sq"].tolist() == [0, 0]
    ctx.set_boundary(BOUNDARY)
    ctx.upload(POS)
    rec = np.zeros(9, y.STATS_DTYPE)
    p = rec.ctypes.data
    one = (_lib.SphxRect * 1)(_lib.SphxRect(0, 0, 1, 1))
    many = (_lib.SphxRect * 9)()

    def err(rc, code, needle):
        assert rc == code and needle in L.sphx_last_error(h).decode(), (rc, L.sphx_last_error(h).decode())

    err(L.sphx_fluid_stats(h, None, 0, 0, None), bad, "out")
    err(L.sphx_fluid_stats(h, None, 1, 0, p), bad, "rects")
    err(L.sphx_fluid_stats(h, many, 9, 0, p), bad, "SPHX_STATS_MAX_RECTS")
    for k in range(4):
        v = [0.0, 0.0, 1.0, 1.0]
        v[k] = float("nan")
        err(L.sphx_fluid_stats(h, (_lib.SphxRect * 1)(_lib.SphxRect(*v)), 1, 0, p), bad, "NaN")
        err(L.sphx_stats_record(h, (_lib.SphxRect * 1)(_lib.SphxRect(*v)), 1, 4, 1), bad, "NaN")
    err(L.sphx_fluid_stats(h, one, 1, 2, p), bad, "flags")
    err(L.sphx_fluid_stats(h, one, 1, 0xFFFFFFFE, p), bad, "flags")
    err(L.sphx_fluid_stats(h, one, 1, _lib.STATS_DEVICE_POINTERS, p | 4), bad, "8-byte aligned")
    assert L.sphx_fluid_stats(h, one, 1, 0, p) == _lib.OK and rec[0]["count"] == 4050
    assert L.sphx_fluid_stats(h, None, 0, 0, p) == _lib.OK  # (rects may be NULL with n_rects == 0)
    err(L.sphx_stats_record(h, None, 1, 4, 1), bad, "rects")
    err(L.sphx_stats_record(h, many, 9, 4, 1), bad, "SPHX_STATS_MAX_RECTS")
    err(L.sphx_stats_record(h, one, 1, 4, 0), bad, "every")
    err(L.sphx_stats_record(h, None, 0, (64 << 20) // 128 + 1, 1), _lib.ERR_CAPACITY, "64 MiB")
    err(L.sphx_stats_record(h, many, 8, (64 << 20) // (9 * 128) + 1, 1), _lib.ERR_CAPACITY, "64 MiB")
    err(L.sphx_stats_record(h, None, 0, 0xFFFFFFFF, 7), _lib.ERR_CAPACITY, "64 MiB")
    assert ctx.stats_status()["recording"] == 0
    assert L.sphx_stats_record(h, None, 0, 0, 0) == _lib.OK  # (stopping takes any `every`)
    assert L.sphx_stats_get_status(h, None) == bad
    ctx.stats_record([(0, 0, 1, 1)], 2)
    err(L.sphx_stats_read(h, 0, 1, p, None), bad, "first_frame + n_frames")
    assert L.sphx_stats_read(h, 0, 0, None, None) == _lib.OK
    timer = y.TimeManager()
    dfsph_step(ctx, timer)
    err(L.sphx_stats_read(h, 0, 1, None, None), bad, "out")
    assert L.sphx_stats_read(h, 0, 1, p, None) == _lib.OK and rec[0]["count"] == 4050  # (info may be NULL)
    # inside a step, for both solvers
    for wcsph in (False, True):
        c = dam_context()
        c.stats_record((), 3)
        if wcsph:
            c.wcsph_step_begin(F(1e-4))
        else:
            c.step_begin(F(1e-4))
        for fn, args in ((c.stats, ()), (c.stats_record, ((), 2)), (c.stats_frames, (0, 0))):
            assert "step_begin" in refused(_lib.ERR_NOT_READY, fn, *args)
        refused(_lib.ERR_NOT_READY, c.download)  # (the call is refused where sphx_download is)
        (c.wcsph_step_finish if wcsph else c.step_finish)(F(1e-4))
        assert c.stats_status() == dict(n_rects=0, recording=1, max_frames=3, every=1, frames=1, dropped=0)
        assert c.stats_frames()[0][0].tobytes() == c.stats().tobytes()
    # after a failed step: allowed wherever sphx_download is
    c = dam_context()
    c.step_begin(F(1e-4))
    refused(bad, c.step_finish, F(-1.0))
    c.download()
    assert c.stats()[0]["count"] == 4050
    # a tile context
    tc = y.SphxContext()
    assert tc.L.sphx_tile_configure(tc.h, 0, 0, 65536, 4, 0, 0) == _lib.OK
    for fn, args in ((tc.stats, ()), (tc.stats_record, ((), 2)), (tc.stats_frames, (0, 0))):
        assert "not available on a tile context" in refused(bad, fn, *args)


# ---- 8. the harness ---------------------------------------------------------------------------------------------------------------------------
def test_harness_stats_out(tmp_path):
    steps, every = 12, 2
    path = tmp_path / "stats.jsonl"
    out = subprocess.run([HARNESS, "--scale", "1", "--steps", str(steps), "--warmup", "0", "--stats-out", str(path), "--stats-every", str(every)],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    assert '"stats_frames": %d' % (steps // every) in out.stdout
    lines = [json.loads(ln) for ln in path.read_text().splitlines()]
    assert len(lines) == steps // every and [ln["step"] for ln in lines] == list(range(every, steps + 1, every))
    w = y.FluidParticleWorld()
    w.reset_fluid(1.0)
    ctx = y.SphxContext()
    ctx.set_boundary(w.boundary_particles)
    ctx.upload(w.positions)
    timer = y.TimeManager()
    dts = []
    for _ in range(steps):
        timer.on_step_started()  # the harness advances the clock like simulation_frame_loop does (timemanager.rs:244-247)
        dfsph_step(ctx, timer, dts)
    r, last = ctx.stats()[0], lines[-1]
    assert last["n"] == ctx.n and F(last["dt"]) == F(dts[-1])
    for k in y.STATS_DTYPE.names:
        if k != "reserved":
            assert np.array_equal(np.asarray(last[k], r[k].dtype), r[k]), k


# ---- 9. physics sanity ------------------------------------------------------------------------------------------------------------------------
def test_a_resting_scene_has_exactly_no_momentum_and_no_kinetic_energy():
    """derived, not measured: every term of sum_vel and sum_speed_sq is +0 when the velocities are zero"""
    pos = np.load(os.path.join(ROOT, "tests", "golden", "uniform_1000.npz"))["in_pos"]
    p = y.default_params()
    p.gravity[0] = p.gravity[1] = 0.0
    ctx = y.SphxContext(p)
    ctx.upload(pos)
    r = ctx.stats([EVERYTHING])
    for g in r:
        assert g["count"] == 1000 and ref.bits(g["sum_vel"]) == [0, 0] and ref.bits(g["sum_speed_sq"]) == [0] and ref.bits(g["max_speed_sq"]) == [0]
        assert ref.bits(g["sum_angular"]) == [0]
    check_all(r, ctx.download(), [EVERYTHING], False, "uniform_1000 at rest")
