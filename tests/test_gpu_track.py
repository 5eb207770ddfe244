"""Following particles by id on the device (include/sphx.h, "following particles by id"): sphx_track_set / _fetch / _record / _read and
sphx_download_by_id against tests/track_reference.py — slot_of from a ctx.download() by the "highest device index wins" rule.  Every
comparison is on raw 32-bit words (NaN patterns and signed zeros included).  The host half of a tracked set, the exports and the NULL
refusals are checked without a GPU in tests/test_track_host.py."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import state_reference as sref
import track_reference as ref
import yasph2d_amd as y
from yasph2d_amd import _lib

pytestmark = pytest.mark.gpu

F = np.float32
INF = float("inf")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "dam_break_4050.npz"))
POS, BOUNDARY = GOLD["in_pos"], GOLD["in_boundary"]
DIAM = F(0.01)
HARNESS = os.path.join(os.path.dirname(os.path.abspath(y.__file__)), "sphx_harness")
CAP = _lib.TRACK_MAX_IDS
A, W = int(ref.ABSENT), int(ref.ABSENT_WORD)
FIELDS = ("slot", "pos", "vel", "density")


def same_words(got, want, what):
    for f in FIELDS:
        g, w = ref.words(got[f]), ref.words(want[f])
        assert g.shape == w.shape, (what, f, g.shape, w.shape)
        bad = np.nonzero(g != w)
        assert bad[0].size == 0, "%s: %s differs at %d of %d words, first at %s: %08x, expected %08x" % (
            what, f, bad[0].size, g.size, tuple(int(b[0]) for b in bad), g[tuple(b[0] for b in bad)], w[tuple(b[0] for b in bad)])


def check_fetch(ctx, ids, d, what):
    ctx.track(ids)
    assert ctx.track_status()["m"] == len(ids)
    same_words(ctx.track_fetch(), ref.fetch(d, ids), what)


def check_by_id(ctx, first, count, d, what):
    got = ctx.download_by_id(first, count)
    want, present = ref.by_id(d, first, count)
    assert got["present"] == present, (what, got["present"], present)
    same_words(got, want, what)
    return got


def refused(code, fn, *args, **kw):
    with pytest.raises(y.SphxError) as e:
        fn(*args, **kw)
    assert e.value.code == code, str(e.value)
    return str(e.value)


def forge(blob, **sections):
    """the blob with whole sections replaced, the section digests and the header digest put right (tests/state_reference.py)"""
    b = np.array(blob, np.uint8, copy=True)
    table = sref.parse_blob(blob)["table"]
    for name, arr in sections.items():
        off, nbytes, _ = table[name]
        raw = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
        assert len(raw) == nbytes
        b[off:off + nbytes] = raw
        at = 168 + 24 * sref.SECTIONS.index(name) + 16
        b[at:at + 8] = np.frombuffer(struct.pack("<Q", sref.digest(raw.tobytes())), np.uint8)
    b[384:392] = np.frombuffer(struct.pack("<Q", sref.digest(b[:384].tobytes())), np.uint8)
    return b


def indexed_context(n, ids=None):
    """n particles that were never stepped (device order = upload order); position, velocity AND density carry the index, so a wrong
    slot shows in every output (the density through a state blob: an upload does not set it)"""
    i = np.arange(n)
    pos = np.stack([F(0.25) + (i % 512) * F(2.0 ** -10), F(0.25) + (i // 512) * F(2.0 ** -10)], -1).astype(F)
    vel = np.stack([i, -i], -1).astype(F)
    ctx = y.SphxContext()
    ctx.upload(pos, vel)
    sections = dict(density=(i + F(0.5)).astype(F))
    if ids is not None:
        sections["particle_id"] = np.asarray(ids, np.uint32)
    ctx.load_state(forge(ctx.save_state(), **sections))
    d = ctx.download()
    assert np.array_equal(d["density"], sections["density"]) and np.array_equal(d["vel"], vel) and np.array_equal(d["pos"], pos)
    return ctx, d


def dfsph_step(ctx, timer):
    vmax = ctx.step_begin(timer.simulation_step(), timer.law(DIAM))
    return ctx.step_finish(y.duration_as_secs_f32(timer.update_simulation_step(DIAM, vmax)))


def wcsph_step(ctx, timer):
    vmax = ctx.wcsph_step_begin(timer.simulation_step())
    return ctx.wcsph_step_finish(y.duration_as_secs_f32(timer.update_simulation_step(DIAM, vmax)))


def dam_context():
    ctx = y.SphxContext()
    ctx.set_boundary(BOUNDARY)
    ctx.upload(POS)
    return ctx


# ---- 1. the look-up against numpy, no stepping ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 4097, 12289])
def test_lookup_against_numpy(n):
    """a wavefront, a workgroup, 16 and 48 workgroups, each with one particle less and one more (and the 1 024-particle trips of the
    look-up with their ragged 16-byte tail)"""
    ctx, d = indexed_context(n)
    assert np.array_equal(d["ids"], np.arange(n))
    up_to_cap = np.arange(min(n, CAP), dtype=np.uint32)
    sets = {
        "all ids up to the cap": up_to_cap, "reversed": up_to_cap[::-1], "every 64th": np.arange(0, n, 64, dtype=np.uint32),
        "first and last only": np.array([0, n - 1], np.uint32), "with duplicates": np.array([n - 1, 0, n // 2, n - 1, n - 1, 0, n // 3], np.uint32),
        "absent ids": np.array([n, 0, n + 1, 0xFFFFFFFF, n - 1], np.uint32), "only absent ids": np.array([n, n + 1, 0xFFFFFFFF], np.uint32),
        "m = 1": np.array([n // 2], np.uint32), "m = 1, the last": np.array([n - 1], np.uint32),
    }
    for name, ids in sets.items():
        check_fetch(ctx, ids, d, "n = %d, %s" % (n, name))
    got = ctx.track_fetch()  # (the last set: one id, present)
    assert got["slot"].tolist() == [n - 1] and got["vel"].tolist() == [[n - 1, -(n - 1)]] and got["density"].tolist() == [n - 0.5]
    # a subset of the outputs, and the id-ordered download of everything, of a window and of nothing
    ctx.track(sets["absent ids"])
    only = ctx.track_fetch(fields=("vel",))
    assert list(only) == ["vel"] and np.array_equal(ref.words(only["vel"]), ref.fetch(d, sets["absent ids"])["vel"])
    everything = check_by_id(ctx, 0, n, d, "n = %d, everything" % n)
    assert everything["present"] == n and np.array_equal(everything["slot"], np.arange(n)) and np.array_equal(everything["vel"], d["vel"])
    assert ctx.download_by_id()["present"] == n  # count=None: the ids issued so far
    check_by_id(ctx, n // 2, n, d, "n = %d, a window half outside" % n)
    empty = ctx.download_by_id(3, 0)
    assert empty["present"] == 0 and empty["pos"].shape == (0, 2)


# ---- 2. the filter under load -----------------------------------------------------------------------------------------------------------
def test_filter_under_load():
    """262 401 = 8 x 128 x 256 + 257 particles (one beyond a full round of the XCD chunk mapping) and the maximum set, whose filter is
    the full 2^18 bits: no result may depend on the filter"""
    n = 8 * 128 * 256 + 257
    ctx, d = indexed_context(n)
    rng = np.random.default_rng(2024)
    sets = {
        "stride 16": (np.arange(CAP, dtype=np.uint32) * 16 + 5), "seeded random": rng.choice(n, CAP, replace=False).astype(np.uint32),
        "the last 16 384": np.arange(n - CAP, n, dtype=np.uint32),
        "half present, half absent, shuffled": rng.permutation(np.concatenate([rng.choice(n, CAP // 2, replace=False), n + rng.choice(1 << 30, CAP // 2, replace=False)])).astype(np.uint32),
        "all absent": (n + np.arange(CAP, dtype=np.uint32) * 262139),
    }
    assert sets["stride 16"].max() < n
    for name, ids in sets.items():
        assert len(ids) == CAP
        check_fetch(ctx, ids, d, name)
    assert (ctx.track_fetch(fields="slot")["slot"] == A).all()  # (the last set)
    check_by_id(ctx, n - 1000, 5000, d, "a window over the end")


# ---- 3. after real re-sorting -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dam60():
    """dam_break_4050 after 60 adaptive steps, its timer and its download: shared, never stepped again"""
    ctx, timer = dam_context(), y.TimeManager()
    for _ in range(60):
        dfsph_step(ctx, timer)
    return ctx, ctx.download()


def test_after_60_steps_host_and_device_path(dam60):
    import torch

    ctx, d = dam60
    n = len(POS)
    assert not np.array_equal(d["ids"], np.arange(n)), "the steps must have re-sorted the particles"
    rng = np.random.default_rng(5)
    for name, ids in (("all", np.arange(n, dtype=np.uint32)), ("random with absent ones", rng.integers(0, n + 500, 3000).astype(np.uint32)),
                      ("three", np.array([0, 17, 4049], np.uint32))):
        check_fetch(ctx, ids, d, name)
        host = ctx.track_fetch()
        inverse = np.full(n + 500, A, np.uint32)
        inverse[:n] = np.argsort(d["ids"])  # (the ids are a permutation of 0 .. n - 1: the slot of id k is argsort(ids)[k])
        assert np.array_equal(host["slot"], inverse[ids]), name  # (ids are unique here: the argsort answer)
        m = len(ids)
        out = {"slot": torch.full((m,), 7, dtype=torch.int32, device="cuda"), "pos": torch.zeros((m, 2), device="cuda"),
               "vel": torch.zeros((m, 2), device="cuda"), "density": torch.zeros(m, device="cuda")}
        assert ctx.track_fetch(out=out) is out
        dev = {"slot": out["slot"].cpu().numpy().view(np.uint32), "pos": out["pos"].cpu().numpy(), "vel": out["vel"].cpu().numpy(),
               "density": out["density"].cpu().numpy()}
        same_words(dev, host, name + ": device-pointer path against host path")
    # the id-ordered download is the particles in upload order
    got = check_by_id(ctx, 0, n, d, "everything")
    order = np.argsort(d["ids"])
    assert got["present"] == n and got["pos"].tobytes() == d["pos"][order].tobytes() and got["density"].tobytes() == d["density"][order].tobytes()
    # ... also through device pointers, out_present included
    slot, pos, present = torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros((n, 2), device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    o = _lib.SphxTrackOut(slot.data_ptr(), pos.data_ptr(), None, None)
    torch.cuda.synchronize()
    ctx._chk(ctx.L.sphx_download_by_id(ctx.h, 0, n, _lib.TRACK_DEVICE_POINTERS, C.byref(o), C.cast(present.data_ptr(), C.POINTER(C.c_uint32))))
    ctx.synchronize()
    assert present.item() == n and np.array_equal(slot.cpu().numpy().view(np.uint32), got["slot"]) and pos.cpu().numpy().tobytes() == got["pos"].tobytes()


# ---- 4. after edits -----------------------------------------------------------------------------------------------------------------------
def test_after_remove_append_and_upload():
    ctx, timer = dam_context(), y.TimeManager()
    n = len(POS)
    for _ in range(20):
        dfsph_step(ctx, timer)
    extra = (np.array([1.2, 1.0], F) + np.stack(np.meshgrid(np.arange(20), np.arange(20)), -1).reshape(-1, 2).astype(F) * F(0.0111)).astype(F)
    ids = np.concatenate([np.arange(0, n, 7), np.arange(n, n + 400, 3), [n + 400, 0xFFFFFFFF]]).astype(np.uint32)  # (set before the edits)
    ctx.track(ids)
    before = ctx.download()
    removed = ctx.remove((0.2, 0.4, 0.7, 0.9))
    assert 0 < removed < n
    d = ctx.download()
    gone = np.setdiff1d(before["ids"], d["ids"])
    assert len(gone) == removed and len(np.intersect1d(gone, ids)) > 10
    got = ctx.track_fetch()
    same_words(got, ref.fetch(d, ids), "after the removal")
    was_removed = np.isin(ids, gone)
    assert (got["slot"][was_removed] == A).all() and (ref.words(got["pos"])[was_removed] == W).all() and (ref.words(got["density"])[was_removed] == W).all()
    assert ctx.append(extra, np.full_like(extra, -1.0)) == n
    d = ctx.download()
    got = ctx.track_fetch()
    same_words(got, ref.fetch(d, ids), "after the append")
    appended = (ids >= n) & (ids < n + 400)
    assert appended.sum() > 100 and (got["slot"][appended] != A).all() and (got["vel"][appended] == -1.0).all() and got["slot"][-2] == A
    issued = n + 400
    assert ctx.ids_issued() == issued
    everything = check_by_id(ctx, 0, issued, d, "download_by_id(0, ids issued)")
    assert everything["present"] == ctx.n == issued - removed
    check_by_id(ctx, issued - 200, 400, d, "a window half outside the issued range")
    check_by_id(ctx, 0xFFFFFF00, 0x100, d, "the last ids there are")
    for s in range(3):  # (the edited set, re-sorted by real steps)
        dfsph_step(ctx, timer)
    d = ctx.download()
    same_words(ctx.track_fetch(), ref.fetch(d, ids), "three steps after the edits")
    check_by_id(ctx, 0, issued, d, "three steps after the edits")
    # sphx_upload renumbers: the set keeps its numbers and now means the new particles
    ctx.upload(POS[:1000], POS[:1000] * F(3.0))
    d = ctx.download()
    assert ctx.track_status()["m"] == len(ids) and ctx.ids_issued() == 1000
    got = ctx.track_fetch()
    same_words(got, ref.fetch(d, ids), "after an upload")
    assert np.array_equal(got["slot"], np.where(ids < 1000, ids, A))


# ---- 5. the recorder against stepping by hand -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver,steps", [("dfsph", 40), ("wcsph", 10)])
def test_recorder_inside_simulation_steps(solver, steps):
    """A records inside ONE simulation_steps(k) call (no hook between the steps), B runs the same steps one by one and downloads"""
    ids = np.array([0, 17, 4049, 2000, 17, 5000, 1], np.uint32)  # (a duplicate and an absent id)
    cls = y.WCSPHSolver if solver == "wcsph" else y.DFSPHSolver
    frames = {}
    for every in (1, 3):
        w = y.FluidParticleWorld()
        w.reset_fluid(1.0)
        a, ta = cls(w), y.TimeManager(cfl_factor=0.2) if solver == "wcsph" else y.TimeManager()
        ctx = a.context()
        ctx.track(ids)
        ctx.track_record(steps, every)
        stats = a.simulation_steps(w, ta, steps, sync_world=False)
        st = ctx.track_status()
        assert (st["m"], st["recording"], st["max_frames"], st["every"], st["frames"], st["dropped"]) == (len(ids), 1, steps, every, steps // every, 0)
        frames[every] = ctx.track_frames()
        assert frames[every].shape == (steps // every, len(ids), 4)
    w = y.FluidParticleWorld()
    w.reset_fluid(1.0)
    b, tb = cls(w), y.TimeManager(cfl_factor=0.2) if solver == "wcsph" else y.TimeManager()
    want = []
    for s in range(steps):
        assert b.simulation_step(w, tb, sync_world=False) == stats[s]
        want.append(ref.frame(b.context().download(), ids))
    want = np.stack(want)
    assert np.array_equal(ref.words(frames[1]), want), "every = 1"
    assert np.array_equal(ref.words(frames[3]), want[2::3]), "every = 3: the frames behind steps 3, 6, ..."
    assert (want[:, 5] == W).all() and np.array_equal(want[:, 1], want[:, 4]) and not np.array_equal(want[0], want[-1])


# ---- 6. no side effects ---------------------------------------------------------------------------------------------------------------------
def test_no_side_effects():
    a, ta, b, tb = dam_context(), y.TimeManager(), dam_context(), y.TimeManager()
    a.track(np.arange(0, 4050, 3, dtype=np.uint32))
    a.track_record(40)
    for s in range(40):
        sa, sb = dfsph_step(a, ta), dfsph_step(b, tb)
        assert sa == sb, "step %d" % s
        assert a.last_flags() == b.last_flags()
        a.track_fetch()
        a.download_by_id(s * 50, 2000)
    assert a.track_status()["frames"] == 40
    assert a.state_digest() == b.state_digest() and len(a.state_digest()) == 9
    assert ta.simulation_step_ns() == tb.simulation_step_ns() and ta.total_simulated_ns == tb.total_simulated_ns
    assert np.array_equal(ref.words(a.track_frames()[-1]), ref.frame(b.download(), np.arange(0, 4050, 3)))


# ---- 7. overflow and status -------------------------------------------------------------------------------------------------------------------
def test_overflow_and_status():
    ctx, timer = dam_context(), y.TimeManager()
    ids = np.array([3, 4049, 9999], np.uint32)
    ctx.track(ids)
    assert ctx.track_status() == dict(m=3, recording=0, max_frames=0, every=0, frames=0, dropped=0)
    ctx.track_record(5)
    want = []
    for s in range(8):
        dfsph_step(ctx, timer)
        want.append(ref.frame(ctx.download(), ids))
    assert ctx.track_status() == dict(m=3, recording=1, max_frames=5, every=1, frames=5, dropped=3)
    assert np.array_equal(ref.words(ctx.track_frames()), np.stack(want[:5]))
    assert np.array_equal(ref.words(ctx.track_frames(2, 2)), np.stack(want[2:4]))
    assert ctx.track_frames(5, 0).shape == (0, 3, 4)
    assert "first_frame + n_frames" in refused(_lib.ERR_INVALID_ARGUMENT, ctx.track_frames, 5, 1)
    refused(_lib.ERR_INVALID_ARGUMENT, ctx.track_frames, 0, 6)
    refused(_lib.ERR_INVALID_ARGUMENT, ctx.track_frames, 0xFFFFFFFF, 2)
    # a failed step takes no frame and does not count
    ctx.track_record(4, 2)  # (a second record resets)
    assert ctx.track_status() == dict(m=3, recording=1, max_frames=4, every=2, frames=0, dropped=0)
    dfsph_step(ctx, timer)
    ctx.step_begin(timer.simulation_step())
    refused(_lib.ERR_INVALID_ARGUMENT, ctx.step_finish, F(-1.0))
    assert ctx.track_status()["frames"] == 0
    dfsph_step(ctx, timer)
    assert ctx.track_status()["frames"] == 1
    assert np.array_equal(ref.words(ctx.track_frames())[0], ref.frame(ctx.download(), ids))
    ctx.track_record(0)  # stop and free
    assert ctx.track_status() == dict(m=3, recording=0, max_frames=0, every=0, frames=0, dropped=0)
    dfsph_step(ctx, timer)
    assert ctx.track_status()["frames"] == 0
    refused(_lib.ERR_INVALID_ARGUMENT, ctx.track_frames, 0, 1)
    ctx.track_record(4)
    dfsph_step(ctx, timer)
    ctx.track(ids[:2])  # a new set discards the recording
    assert ctx.track_status() == dict(m=2, recording=0, max_frames=0, every=0, frames=0, dropped=0)
    ctx.track([])
    assert ctx.track_status()["m"] == 0 and ctx.track_fetch()["slot"].shape == (0,)


# ---- 8. repeated ids ----------------------------------------------------------------------------------------------------------------------------
def test_repeated_ids_give_the_higher_slot():
    """sphx_state_load accepts a blob whose id section repeats an id: slot_of is then the highest slot, on every call"""
    ids = np.arange(256, dtype=np.uint32)
    ids[5] = ids[250] = 77  # id 77 at the slots 5, 77 and 250; the ids 5 and 250 are gone
    ctx, d = indexed_context(256, ids)
    assert np.array_equal(d["ids"], ids)
    for _ in range(3):
        got = ctx.download_by_id(0, 256)
        same_words(got, ref.by_id(d, 0, 256)[0], "download_by_id")
        assert got["slot"][77] == 250 and got["slot"][5] == A and got["slot"][250] == A and got["present"] == 254
        ctx.track([77, 5, 250, 76, 77])
        got = ctx.track_fetch()
        same_words(got, ref.fetch(d, [77, 5, 250, 76, 77]), "fetch")
        assert got["slot"].tolist() == [250, A, A, 76, 250] and got["density"][0] == 250.5


# ---- 9. every refusal in the contract ---------------------------------------------------------------------------------------------------------
def test_refusals():
    ctx = y.SphxContext()
    L, h, bad = ctx.L, ctx.h, _lib.ERR_INVALID_ARGUMENT
    # before any upload: success, everything absent
    ctx.track([0, 1, 2])
    got = ctx.track_fetch()
    assert (got["slot"] == A).all() and (ref.words(got["pos"]) == W).all() and (ref.words(got["vel"]) == W).all() and (ref.words(got["density"]) == W).all()
    got = ctx.download_by_id(0, 10)
    assert got["present"] == 0 and (got["slot"] == A).all() and (ref.words(got["density"]) == W).all()
    assert ctx.download_by_id()["slot"].shape == (0,)
    ctx.set_boundary(BOUNDARY)
    ctx.upload(POS)
    buf = np.zeros(64, F)
    p = buf.ctypes.data
    o = _lib.SphxTrackOut(p, None, None, None)
    none = _lib.SphxTrackOut()
    ids = (C.c_uint32 * 4)(1, 2, 3, 4)

    def err(rc, code, needle):
        assert rc == code and needle in L.sphx_last_error(h).decode(), (rc, L.sphx_last_error(h).decode())

    err(L.sphx_track_set(h, ids, CAP + 1), bad, "SPHX_TRACK_MAX_IDS")
    err(L.sphx_track_set(h, None, 4), bad, "ids")
    assert ctx.track_status()["m"] == 3  # (a refused set leaves the old one)
    err(L.sphx_track_fetch(h, 0, None), bad, "out")
    err(L.sphx_track_fetch(h, 0, C.byref(none)), bad, "every pointer is NULL")
    err(L.sphx_track_fetch(h, 2, C.byref(o)), bad, "flags")
    err(L.sphx_download_by_id(h, 0, 4, 0, None, None), bad, "out")
    err(L.sphx_download_by_id(h, 0, 4, 0, C.byref(none), None), bad, "every pointer is NULL")
    err(L.sphx_download_by_id(h, 0, 4, 4, C.byref(o), None), bad, "flags")
    err(L.sphx_download_by_id(h, 2, 0xFFFFFFFF, 0, C.byref(o), None), bad, "first_id + count")
    err(L.sphx_download_by_id(h, 0xFFFFFFFF, 2, 0, C.byref(o), None), bad, "first_id + count")
    assert L.sphx_download_by_id(h, 0xFFFFFFFF, 1, 0, C.byref(o), None) == _lib.OK and buf.view(np.uint32)[0] == A  # up to 2^32: fine
    assert L.sphx_download_by_id(h, 0, 4, 0, C.byref(o), None) == _lib.OK  # out_present may be NULL
    err(L.sphx_track_read(h, 0, 0, 8, p), bad, "flags")
    assert L.sphx_track_get_status(h, None) == bad
    err(L.sphx_track_record(h, 10, 0), bad, "every")
    ctx.track(np.arange(CAP, dtype=np.uint32))
    err(L.sphx_track_record(h, 4097, 1), _lib.ERR_CAPACITY, "1 GiB")
    err(L.sphx_track_record(h, 0xFFFFFFFF, 7), _lib.ERR_CAPACITY, "1 GiB")
    assert ctx.track_status()["recording"] == 0
    ctx.track([])
    err(L.sphx_track_record(h, 10, 1), _lib.ERR_NOT_READY, "empty")
    assert L.sphx_track_record(h, 0, 1) == _lib.OK  # (stopping needs no set)
    # inside a step, for both solvers
    for wcsph in (False, True):
        c = dam_context()
        c.track([5, 6])
        c.track_record(3)
        if wcsph:
            c.wcsph_step_begin(F(1e-4))
        else:
            c.step_begin(F(1e-4))
        for fn, args in ((c.track, ([1],)), (c.track_fetch, ()), (c.track_record, (2,)), (c.track_frames, (0, 0)), (c.download_by_id, (0, 4))):
            assert "step_begin" in refused(_lib.ERR_NOT_READY, fn, *args)
        (c.wcsph_step_finish if wcsph else c.step_finish)(F(1e-4))
        assert c.track_status() == dict(m=2, recording=1, max_frames=3, every=1, frames=1, dropped=0)
        assert np.array_equal(ref.words(c.track_frames())[0], ref.frame(c.download(), [5, 6]))
    # a tile context
    tc = y.SphxContext()
    assert tc.L.sphx_tile_configure(tc.h, 0, 0, 65536, 4, 0, 0) == _lib.OK
    for fn, args in ((tc.track, ([1],)), (tc.track_fetch, ()), (tc.track_record, (2,)), (tc.track_frames, (0, 0)), (tc.download_by_id, (0, 4))):
        assert "not available on a tile context" in refused(bad, fn, *args)


# ---- 10. the harness ----------------------------------------------------------------------------------------------------------------------------
def test_harness_track_csv_equals_the_python_recorder(tmp_path):
    steps, ids = 20, [0, 17, 4049]
    path = tmp_path / "track.csv"
    out = subprocess.run([HARNESS, "--scale", "1", "--steps", str(steps), "--warmup", "0", "--track", ",".join(map(str, ids)), "--track-out", str(path)],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    assert '"track_frames": %d' % steps in out.stdout
    lines = path.read_text().splitlines()
    assert lines[0] == "frame,id,x,y,vx,vy" and len(lines) == 1 + steps * len(ids)
    csv = np.array([[float(v) for v in ln.split(",")] for ln in lines[1:]])
    assert np.array_equal(csv[:, 0], np.repeat(np.arange(steps), len(ids))) and np.array_equal(csv[:, 1], np.tile(ids, steps))
    w = y.FluidParticleWorld()
    w.reset_fluid(1.0)
    ctx = y.SphxContext()
    ctx.set_boundary(w.boundary_particles)
    ctx.upload(w.positions)
    ctx.track(ids)
    ctx.track_record(steps)
    timer = y.TimeManager()
    for _ in range(steps):
        timer.on_step_started()  # the harness advances the clock like simulation_frame_loop does (timemanager.rs:244-247)
        dfsph_step(ctx, timer)
    frames = ctx.track_frames()
    assert np.array_equal(ref.words(csv[:, 2:].astype(F)).reshape(steps, len(ids), 4), ref.words(frames))
