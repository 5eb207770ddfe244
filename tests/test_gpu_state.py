"""Saving and restoring a context on the GPU (sphx_state_*, include/sphx.h): the digest kernel against its numpy restatement, the blob's
contents, and the promise — a context that loads a blob and receives the same calls produces the same bits — against the oracle's
committed answers (tests/golden), against an untouched twin, across processes and through device memory.  Everything is bit-exact."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest
import state_reference as ref
from test_golden import check_state, check_wcsph, load
from util import assert_bits_equal, lattice_scene

import yasph2d_amd as y
from yasph2d_amd import _lib

pytestmark = pytest.mark.gpu

DIAM = np.float32(0.01)
HARNESS = os.path.join(os.path.dirname(os.path.abspath(y.__file__)), "sphx_harness")
IT_KEYS = ("density_iterations", "divergence_iterations", "warmstart_density", "warmstart_divergence")


def dfsph_step(ctx, timer, law=False):
    vmax = ctx.step_begin(timer.simulation_step(), timer.law(DIAM) if law else None)
    dt_ns = timer.update_simulation_step(DIAM, vmax)
    return ctx.step_finish(y.duration_as_secs_f32(dt_ns)), dt_ns


def wcsph_step(ctx, timer):
    vmax = ctx.wcsph_step_begin(timer.simulation_step())
    dt_ns = timer.update_simulation_step(DIAM, vmax)
    return ctx.wcsph_step_finish(y.duration_as_secs_f32(dt_ns)), dt_ns


def timer_like(timer):
    """A fresh TimeManager (of another kind) that takes over `timer`'s state."""
    t = y.TimeManager(fixed_ns=1)
    t.set_state(timer.get_state())
    return t


def full_state(ctx):
    d = ctx.download()
    d.update(ctx.download_solver_state())
    c, _, l = ctx.download_neighbors()
    d.update(nb_counts=c, nb_lists=l)
    return d


def assert_same_arrays(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), f"{what}: {k} differs"


def refused(code, fn, *args):
    with pytest.raises(y.SphxError) as e:
        fn(*args)
    assert e.value.code == code, str(e.value)
    return str(e.value)


def dam_context(g, **kw):
    ctx = y.SphxContext(y.default_params(fixed_iterations=tuple(int(v) for v in g["fixed"]), **kw))
    ctx.set_boundary(g["in_boundary"])
    ctx.upload(g["in_pos"])
    return ctx


@pytest.fixture(scope="module")
def dam():
    return load("dam_break_4050.npz")


@pytest.fixture(scope="module")
def dam100(dam):
    """The golden scene after 100 adaptive steps (the oracle's s100_*: alpha, kappa and stiffness are all live there; for the first steps
    of the free fall kappa and stiffness are still zero), its timer, and its blob: shared, never stepped again."""
    ctx, timer = dam_context(dam), y.TimeManager()
    stats = [dfsph_step(ctx, timer)[0] for _ in range(100)]
    return ctx, timer, stats, ctx.save_state()


# ---- 1. the digest kernel against numpy -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 1023, 1025, 4050, 300001])
def test_digest_kernel_after_upload(n):
    """Odd counts, a ragged tail behind the 16-byte loads (n = 1: two words; 4-byte sections of odd n), one and many workgroups."""
    ctx = y.SphxContext()
    rng = np.random.default_rng(n)
    for b in (0, 1, 65):
        pos, bnd = lattice_scene(n, b)
        vel = rng.standard_normal((n, 2)).astype(np.float32)
        ctx.set_boundary(bnd)
        ctx.upload(pos, vel)
        d, ss = ctx.download(), ctx.download_solver_state()
        assert_bits_equal(d["pos"], pos, "uploaded positions")
        want = ref.state_digests(d["pos"], d["vel"], d["ids"], d["density"], ss["alpha"][:0], ss["kappa"][:0], ss["stiffness"][:0],
                                 np.zeros((0, 2), np.float32), bnd)
        got = ctx.state_digest()
        assert got == want, (n, b, {k: (hex(got[k]), hex(want[k])) for k in got if got[k] != want[k]})
        assert got["alpha"] == 0 and (got["positions"] != got["velocities"] or n == 0)


# ---- 2. the blob ----------------------------------------------------------------------------------------------------------------------------
def test_blob_contents(dam, dam100):
    ctx, timer, stats, blob = dam100
    assert blob.dtype == np.uint8 and len(blob) == ctx.state_size()
    p = ref.parse_blob(blob)
    d, ss = ctx.download(), ctx.download_solver_state()
    n = len(dam["in_pos"])
    assert (p["n"], p["b"], p["cached_n"], p["wcsph_n"], p["ids_issued"]) == (n, len(dam["in_boundary"]), n, 0, n)
    assert (p["num_density_iters"], p["num_divergence_iters"]) == (stats[-1]["density_iterations"], stats[-1]["divergence_iterations"])
    assert (p["set_changed"], p["tiling_invariant"], p["lists_current"], p["sampling_allowed"]) == (0, 0, 1, 1)
    assert p["params_bytes"][:60] == bytes(ctx.params)[:60] and p["params"]["fixed_density_iterations"] == 0
    for name, a in (("positions", d["pos"]), ("velocities", d["vel"]), ("particle_id", d["ids"]), ("density", d["density"]),
                    ("alpha", ss["alpha"]), ("kappa", ss["kappa"]), ("stiffness", ss["stiffness"]), ("boundary", dam["in_boundary"])):
        assert p[name].tobytes() == np.ascontiguousarray(a).tobytes(), name
    for name in ("alpha", "kappa", "stiffness"):  # (the oracle's answer, where all three are non-zero)
        assert p[name].tobytes() == dam[f"s100_{name}"].tobytes() and np.abs(dam[f"s100_{name}"]).max() > 0, name
    live = ctx.state_digest()
    assert {s: p["table"][s][2] for s in ref.SECTIONS} == live
    assert live == ref.state_digests(d["pos"], d["vel"], d["ids"], d["density"], ss["alpha"], ss["kappa"], ss["stiffness"], p["accel"], dam["in_boundary"])
    assert ctx.save_state().tobytes() == blob.tobytes(), "two saves of one state must be byte-identical"
    dev = ctx.save_state(device=True)
    assert dev.is_cuda and dev.cpu().numpy().tobytes() == blob.tobytes(), "the device path writes the same bytes"


# ---- 3. - 5. resume against the oracle's recorded answers -----------------------------------------------------------------------------------------
def test_adaptive_resume_matches_golden(dam):
    g = dam
    a, ta = dam_context(g), y.TimeManager()
    for _ in range(70):
        dfsph_step(a, ta)
    blob = a.save_state()
    b, tb = y.SphxContext(y.default_params()), timer_like(ta)
    b.load_state(blob)
    its = []
    for _ in range(70, 100):
        st, dt_ns = dfsph_step(b, tb)
        its.append([st[k] for k in IT_KEYS])
    its = np.array(its, np.uint32)
    np.testing.assert_array_equal(its, g["iterations"][70:100])
    assert (its[:, 3] == 1).any(), "the continued window must contain a divergence warm start (the fixture guarantees it)"
    s = full_state(b)
    check_state(g, 100, s["pos"], s["vel"], s["density"], s["ids"], s["alpha"], s["kappa"], s["stiffness"], s["nb_counts"], s["nb_lists"], dt_ns)


def test_fixed_resume_matches_golden():
    g = load("dam_break_4050_fixed.npz")
    a, ta = dam_context(g), y.TimeManager()
    for _ in range(10):
        dfsph_step(a, ta)
    b, tb = y.SphxContext(y.default_params(fixed_iterations=(3, 2))), timer_like(ta)
    b.load_state(a.save_state().tobytes())  # (bytes: the third kind of blob load_state takes)
    its = []
    for _ in range(10, 20):
        st, dt_ns = dfsph_step(b, tb)
        its.append([st[k] for k in IT_KEYS])
    np.testing.assert_array_equal(np.array(its, np.uint32), g["iterations"][10:20])
    assert all(row[2] == 1 and row[3] == 1 for row in its), "both warm starts fire on every step after the first"
    s = full_state(b)
    check_state(g, 20, s["pos"], s["vel"], s["density"], s["ids"], s["alpha"], s["kappa"], s["stiffness"], s["nb_counts"], s["nb_lists"], dt_ns)


def test_wcsph_resume_matches_golden():
    g = load("wcsph_dam_break_4050.npz")
    a = y.SphxContext()
    a.set_boundary(g["in_boundary"])
    a.upload(g["in_pos"])
    ta = y.TimeManager(timestep_max_ns=int(g["timestep_max_ns"]), timestep_min_ns=int(g["timestep_min_ns"]), cfl_factor=0.2)
    for _ in range(50):
        wcsph_step(a, ta)
    blob = a.save_state()
    p = ref.parse_blob(blob)
    assert p["wcsph_n"] == len(g["in_pos"]) and p["cached_n"] == 0 and np.abs(p["accel"]).max() > 0
    b, tb = y.SphxContext(), timer_like(ta)
    b.load_state(blob)
    for _ in range(50, 300):
        _, dt_ns = wcsph_step(b, tb)
    d = b.download()
    c, _, l = b.download_neighbors()
    check_wcsph(g, 300, d["pos"], d["vel"], d["density"], d["ids"], c, l, dt_ns)


# ---- 6. another process ---------------------------------------------------------------------------------------------------------------------
def test_resume_in_another_process(tmp_path):
    def run(*args):
        out = subprocess.run([HARNESS, "--solver", "dfsph", "--scale", "1", "--warmup", "0"] + [str(a) for a in args], capture_output=True, text=True,
                             timeout=600)
        assert out.returncode == 0, out.stderr
        return json.loads(out.stdout.strip().splitlines()[-1])

    whole, part, rest = tmp_path / "whole.sphx", tmp_path / "part.sphx", tmp_path / "rest.sphx"
    r1 = run("--steps", 100, "--save-state", whole)
    run("--steps", 70, "--save-state", part)
    r3 = run("--load-state", part, "--steps", 30, "--save-state", rest)
    assert whole.read_bytes() == rest.read_bytes(), "100 steps, and 70 steps + a file + 30 steps in another process, must end in the same bytes"
    assert whole.read_bytes() != part.read_bytes()
    for k in ("state_fnv1a", "timer_step_ns", "simulated_ns", "particles", "boundary"):
        assert r1[k] == r3[k], k
    # --save-state FILE:at=STEP writes the same file mid-run
    mid = tmp_path / "mid.sphx"
    run("--steps", 75, "--save-state", f"{mid}:at=70")
    assert mid.read_bytes() == part.read_bytes()


# ---- 7. rollback in one context through device memory ---------------------------------------------------------------------------------------
def test_rollback_through_device_memory(dam):
    ctx, timer = dam_context(dam), y.TimeManager()
    for _ in range(5):
        dfsph_step(ctx, timer, law=True)
    blob, tstate = ctx.save_state(device=True), timer.get_state()
    assert blob.is_cuda and blob.numel() == ctx.state_size()
    rec = [dfsph_step(ctx, timer, law=True) for _ in range(5)]
    want = full_state(ctx)
    ctx.load_state(blob)  # (the fifth step's finish has queued a run-ahead pass: load drops it)
    timer.set_state(tstate)
    assert [dfsph_step(ctx, timer, law=True) for _ in range(5)] == rec
    assert_same_arrays(full_state(ctx), want, "after the rollback")


# ---- 8. edits travel ------------------------------------------------------------------------------------------------------------------------
def test_edits_travel(dam):
    a, ta = dam_context(dam), y.TimeManager()
    for _ in range(10):
        dfsph_step(a, ta)
    k = a.remove((-np.inf, -np.inf, 0.15, np.inf))
    assert 0 < k < a.n
    side = int(np.ceil(np.sqrt(k)))
    grid = np.stack(np.meshgrid(np.arange(side), np.arange(side)), -1).reshape(-1, 2)[:k].astype(np.float32)
    first = a.append(np.array([1.0, 1.0], np.float32) + grid * np.float32(1.0 / 90.0))
    assert first == len(dam["in_pos"]) and a.n == len(dam["in_pos"])  # the count is back at cached_n: only the mark says "another set"
    blob = a.save_state()
    p = ref.parse_blob(blob)
    assert (p["set_changed"], p["lists_current"], p["sampling_allowed"], p["cached_n"], p["ids_issued"]) == (1, 0, 0, a.n, a.n + k)
    b, tb = y.SphxContext(), timer_like(ta)
    b.load_state(blob)
    assert b.save_state().tobytes() == blob.tobytes()
    for s in range(6):
        (sa, na), (sb, nb) = dfsph_step(a, ta), dfsph_step(b, tb)
        assert sa == sb and na == nb, s
        assert bool(sa["flags"] & y.FLAG_WARMUP) == (s == 0), "the step after the edit runs the warm-up block, in both"
    assert_same_arrays(full_state(a), full_state(b), "after the edit and six steps")
    empty = np.zeros((0, 2), np.float32)
    assert a.append(empty) == b.append(empty) == len(dam["in_pos"]) + k


# ---- 9. sampling and rendering after a load -----------------------------------------------------------------------------------------------------
def test_sample_and_render_after_load(dam, dam100):
    a, _, _, blob = dam100
    b = y.SphxContext()
    b.load_state(blob)
    pts = np.random.default_rng(5).uniform((0.0, 0.6), (0.7, 1.8), (2000, 2)).astype(np.float32)
    assert_same_arrays(a.sample(pts), b.sample(pts), "sample after load")
    ia, oa = a.render(width=320, height=180, owner=True)
    ib, ob = b.render(width=320, height=180, owner=True)
    assert ia.tobytes() == ib.tobytes() and oa.tobytes() == ob.tobytes() and (oa < _lib.RENDER_BOUNDARY).any()
    assert_same_arrays(full_state(a), full_state(b), "lists and arrays right after the load")
    # a blob saved right after an upload: sampling was not allowed in the saver, and is not after the load
    u = dam_context(dam)
    assert "sphx_upload" in refused(_lib.ERR_NOT_READY, u.sample, pts[:4])
    fresh = ref.parse_blob(u.save_state())
    assert (fresh["lists_current"], fresh["sampling_allowed"], fresh["cached_n"]) == (0, 0, 0)
    v = y.SphxContext()
    v.load_state(u.save_state())
    refused(_lib.ERR_NOT_READY, v.sample, pts[:4])
    tu, tv = y.TimeManager(), y.TimeManager()
    assert dfsph_step(u, tu) == dfsph_step(v, tv)
    assert_same_arrays(full_state(u), full_state(v), "first step after upload / after loading an uploaded state")


# ---- 10. no side effects ---------------------------------------------------------------------------------------------------------------------
def test_save_and_digest_leave_the_run_alone(dam):
    g = dam
    ctx, timer = dam_context(g), y.TimeManager()
    its, sizes = [], set()
    for s in range(10):
        st, dt_ns = dfsph_step(ctx, timer, law=True)
        its.append([st[k] for k in IT_KEYS])
        blob = ctx.save_state()
        assert {k: ref.parse_blob(blob)["table"][k][2] for k in ref.SECTIONS} == ctx.state_digest()
        sizes.add(len(blob))
    assert len(sizes) == 1
    np.testing.assert_array_equal(np.array(its, np.uint32), g["iterations"][:10])
    s = full_state(ctx)
    check_state(g, 10, s["pos"], s["vel"], s["density"], s["ids"], s["alpha"], s["kappa"], s["stiffness"], s["nb_counts"], s["nb_lists"], dt_ns)


# ---- 11. refusals that leave the context untouched ------------------------------------------------------------------------------------------------
def test_refused_loads_leave_the_context_untouched(dam, dam100):
    _, _, _, good = dam100
    a, ta = dam_context(dam), y.TimeManager()
    twin, tt = dam_context(dam), y.TimeManager()
    for _ in range(3):
        assert dfsph_step(a, ta) == dfsph_step(twin, tt)

    def forged(**patch):
        b = good.copy()
        for off, raw in patch.values():
            b[off:off + len(raw)] = np.frombuffer(raw, np.uint8)
        return b

    other_mu = dam_context(dam, fluid_viscosity=0.5).save_state()
    ti = dam_context(dam)
    ti.set_tiling_invariant(True)
    cases = [("truncated by 8 bytes", good[:-8], "truncated"), ("truncated inside the header", good[:100], "truncated"),
             ("empty", good[:0], "truncated"), ("one byte too long", np.concatenate([good, np.zeros(1, np.uint8)]), "longer"),
             ("bad magic", forged(m=(0, b"SPHXSTAt")), "magic"), ("a future version", forged(v=(8, (2).to_bytes(4, "little"))), "version"),
             ("a header scalar changed", forged(s=(152, (1).to_bytes(4, "little"))), "header"),
             ("another fluid_viscosity", other_mu, "fluid_viscosity"), ("saved in tiling-invariant mode", ti.save_state(), "tiling-invariant")]
    for what, blob, needle in cases:
        msg = refused(_lib.ERR_INVALID_ARGUMENT, a.load_state, blob)
        assert needle in msg, (what, msg)
        assert a.state_digest() == twin.state_digest(), what
        assert dfsph_step(a, ta) == dfsph_step(twin, tt), what
    # the other way round: a context in tiling-invariant mode refuses a blob saved outside it, and stays what it was
    before = ti.state_digest()
    assert "tiling-invariant" in refused(_lib.ERR_INVALID_ARGUMENT, ti.load_state, good)
    assert ti.state_digest() == before
    assert_same_arrays(full_state(a), full_state(twin), "after nine refusals")


# ---- 12. a flipped payload byte ---------------------------------------------------------------------------------------------------------------
def test_flipped_payload_byte(dam, dam100):
    src, tsrc, _, good = dam100
    table = ref.parse_blob(good)["table"]
    ctx = dam_context(dam)
    for section in ("velocities", "kappa"):
        bad = good.copy()
        off, nbytes, _ = table[section]
        bad[off + nbytes // 2] ^= 0x10
        msg = refused(_lib.ERR_INVALID_ARGUMENT, ctx.load_state, bad)
        assert section in msg and "digest" in msg, msg
        refused(_lib.ERR_NOT_READY, ctx.step_begin, np.float32(1e-4))
        refused(_lib.ERR_NOT_READY, ctx.save_state)
    # the boundary is checked on the host before anything changes
    bad = good.copy()
    bad[table["boundary"][0] + 5] ^= 0x01
    assert "boundary" in refused(_lib.ERR_INVALID_ARGUMENT, ctx.load_state, bad)
    ctx.load_state(good)  # a good load repairs the context
    assert ctx.save_state().tobytes() == good.tobytes()
    twin, tt = y.SphxContext(), timer_like(tsrc)
    twin.load_state(good)
    tc = timer_like(tsrc)
    for _ in range(3):
        assert dfsph_step(ctx, tc) == dfsph_step(twin, tt)
    assert_same_arrays(full_state(ctx), full_state(twin), "after the repair")


# ---- 13. other refusals -----------------------------------------------------------------------------------------------------------------------
def test_other_refusals(dam, dam100):
    _, _, _, good = dam100
    ctx = y.SphxContext()
    assert "no state" in refused(_lib.ERR_NOT_READY, ctx.save_state)  # before any upload
    refused(_lib.ERR_NOT_READY, ctx.state_digest)
    ctx.set_boundary(dam["in_boundary"])
    ctx.upload(dam["in_pos"])
    timer = y.TimeManager()
    vmax = ctx.step_begin(timer.simulation_step())
    for fn, args in ((ctx.save_state, ()), (ctx.state_digest, ()), (ctx.load_state, (good,)), (ctx.state_size, ())):
        assert "step_begin" in refused(_lib.ERR_NOT_READY, fn, *args)
    ctx.step_finish(y.duration_as_secs_f32(timer.update_simulation_step(DIAM, vmax)))
    wc = dam_context(dam)  # (the WCSPH step is a step too)
    wc.wcsph_step_begin(np.float32(1e-4))
    refused(_lib.ERR_NOT_READY, wc.save_state)
    wc.wcsph_step_finish(np.float32(1e-4))
    assert ref.parse_blob(wc.save_state())["wcsph_n"] == wc.n
    # a capacity that is too small: SPHX_ERR_CAPACITY, the needed size reported, nothing written
    size, need = ctx.state_size(), C.c_uint64()
    buf = np.full(size, 0xAB, np.uint8)
    assert ctx.L.sphx_state_save(ctx.h, buf.ctypes.data_as(C.c_void_p), size - 1, 0, C.byref(need)) == _lib.ERR_CAPACITY
    assert need.value == size and (buf == 0xAB).all()
    assert ctx.L.sphx_state_save(ctx.h, None, 0, 0, C.byref(need)) == _lib.ERR_INVALID_ARGUMENT and need.value == size
    assert ctx.L.sphx_state_save(ctx.h, buf.ctypes.data_as(C.c_void_p), size, 2, None) == _lib.ERR_INVALID_ARGUMENT  # unknown flag bit
    assert ctx.L.sphx_state_load(ctx.h, buf.ctypes.data_as(C.c_void_p), size, 2) == _lib.ERR_INVALID_ARGUMENT
    assert ctx.L.sphx_state_save(ctx.h, buf.ctypes.data_as(C.c_void_p), size, 0, None) == _lib.OK and ref.parse_blob(buf)["n"] == ctx.n
    # a tile context
    tc = y.SphxContext()
    assert tc.L.sphx_tile_configure(tc.h, 0, 0, 65536, 4, 0, 0) == _lib.OK
    for fn, args in ((tc.save_state, ()), (tc.state_digest, ()), (tc.load_state, (good,))):
        assert "not available on a tile context" in refused(_lib.ERR_INVALID_ARGUMENT, fn, *args)
    # files
    assert "cannot open" in refused(_lib.ERR_INVALID_ARGUMENT, ctx.load_state_file, "/nonexistent/dir/state.sphx")
    assert "cannot write" in refused(_lib.ERR_INVALID_ARGUMENT, ctx.save_state_file, "/nonexistent/dir/state.sphx")


# ---- the files and the solver object ------------------------------------------------------------------------------------------------------------
def test_state_file_and_solver_object(tmp_path, dam100):
    src, _, _, good = dam100
    path = tmp_path / "ctx.sphx"
    src.save_state_file(path)
    assert path.read_bytes() == good.tobytes() and not os.path.exists(str(path) + ".tmp")
    c = y.SphxContext()
    c.load_state_file(path)
    assert c.save_state().tobytes() == good.tobytes()
    # DFSPHSolver.save / load: the context and the timer in one file; the world follows the device
    w = y.FluidParticleWorld()
    w.reset_fluid(1.0)
    solver, timer = y.DFSPHSolver(w), y.TimeManager()
    run = tmp_path / "run.sphx"
    assert "step first" in refused(_lib.ERR_NOT_READY, solver.save, w, timer, run)
    solver.simulation_steps(w, timer, 20, sync_world=False)
    solver.save(w, timer, run)
    rest = solver.simulation_steps(w, timer, 10, sync_world=True)
    w2 = y.FluidParticleWorld()
    solver2, timer2 = y.DFSPHSolver(w2), y.TimeManager(fixed_ns=5)
    solver2.load(w2, timer2, run)
    assert w2.num_dynamic_particles == w.num_dynamic_particles and w2.boundary_particles.tobytes() == w.boundary_particles.tobytes()
    assert timer2.num_steps == 20
    assert solver2.simulation_steps(w2, timer2, 10, sync_world=True) == rest
    assert w2.positions.tobytes() == w.positions.tobytes() and w2.velocities.tobytes() == w.velocities.tobytes()
    assert w2.particle_ids.tobytes() == w.particle_ids.tobytes() and bytes(timer2.get_state()) == bytes(timer.get_state())
    # a damaged file is refused as a whole: world and timer stay as they are
    raw = bytearray(run.read_bytes())
    raw = raw[:-16]
    (tmp_path / "bad.sphx").write_bytes(bytes(raw))
    before = bytes(timer2.get_state())
    assert "truncated" in refused(_lib.ERR_INVALID_ARGUMENT, solver2.load, w2, timer2, tmp_path / "bad.sphx")
    assert bytes(timer2.get_state()) == before
    # the multi-GPU solver object has no counterpart yet
    m = y.DFSPHMultiSolver(w, devices=[0, 0])
    assert "multi-GPU" in refused(_lib.ERR_INVALID_ARGUMENT, m.save, w, timer, tmp_path / "multi.sphx")
    assert "multi-GPU" in refused(_lib.ERR_INVALID_ARGUMENT, m.load, w, timer, run)
