"""Per-particle flow fields on the device (sphx_particle_fields): bit equality with the float32 restatement of the contract
(tests/fields_reference.py) on every path and for every subset of the outputs, over both list formats, capped lists and the size edges;
the float64 bound; the analytic gradient of linear velocity fields; the state rules and argument errors of include/sphx.h; no side
effects on a run; and the harness's --fields-out."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import fields_reference as fr
import yasph2d_amd as y
from util import dam_break, lattice_scene, uniform_points
from yasph2d_amd import _lib

pytestmark = pytest.mark.gpu

F = np.float32
DIAM = F(0.01)
HARNESS = os.path.join(os.path.dirname(os.path.abspath(y.__file__)), "sphx_harness")
NAMES = fr.NAMES
SHAPE = dict(vel_grad=(2, 2), divergence=(), vorticity=(), color_grad=(2,))


def dfsph_step(ctx, timer):
    vmax = ctx.step_begin(timer.simulation_step(), timer.law(DIAM))
    return vmax, ctx.step_finish(y.duration_as_secs_f32(timer.update_simulation_step(DIAM, vmax)))


def wcsph_step(ctx, timer):
    vmax = ctx.wcsph_step_begin(timer.simulation_step())
    return vmax, ctx.wcsph_step_finish(y.duration_as_secs_f32(timer.update_simulation_step(DIAM, vmax)))


def scene_ctx(scale=1.0, **kw):
    pos, bnd = dam_break(scale)
    ctx = y.SphxContext(**kw)
    ctx.set_boundary(bnd)
    ctx.upload(pos)
    return ctx


def built_ctx(pos, bnd=None, vel=None, **kw):
    """a context whose lists and densities belong to the uploaded positions without a step (update_neighborhood + update_densities)"""
    ctx = y.SphxContext(**kw)
    if bnd is not None and len(bnd):
        ctx.set_boundary(bnd)
    ctx.upload(pos, vel)
    ctx.update_neighborhood()
    ctx.update_densities(y.KERNEL_WENDLAND_C2)
    return ctx


def state_of(ctx):
    d = ctx.download()
    counts, _, lists = ctx.download_neighbors()
    return dict(pos=d["pos"], vel=d["vel"], density=d["density"], boundary=ctx.download_boundary()[0], ids=d["ids"]), counts, lists


def consts_of(ctx):
    K = fr.Constants(ctx.params, ctx.constants())
    K0 = fr.Constants(ctx.params)  # (the restated derivation agrees with the device's constants)
    assert (K0.w_hinv, K0.w_ngrad) == (K.w_hinv, K.w_ngrad)
    return K


def assert_bits(dev, ref, what):
    for f in dev:
        a, b = np.asarray(dev[f], F), np.asarray(ref[f], F)
        assert a.shape == b.shape, (what, f, a.shape, b.shape)
        bad = a.view(np.uint32) != b.view(np.uint32)
        assert not bad.any(), "%s: %s differs in %d of %d words, first at %s" % (what, f, int(bad.sum()), bad.size, np.argwhere(bad)[0].tolist())


def device_path(ctx, names=NAMES):
    """sphx_particle_fields with SPHX_FIELDS_DEVICE_POINTERS into torch outputs (pre-filled with NaN: an unwritten entry shows)"""
    import torch

    n = ctx.n
    out = {f: torch.full((n,) + SHAPE[f], float("nan"), dtype=torch.float32, device="cuda") for f in names}
    assert ctx.fields(out=out) is out
    return {f: t.cpu().numpy() for f, t in out.items()}


def check_state(ctx, what, torch_too=True, bound=True):
    """every output on both paths, every single output, two subsets: bit for bit against the restatement; and the float64 bound"""
    st, counts, lists = state_of(ctx)
    K = consts_of(ctx)
    ref = fr.fields32(K, st, counts, lists)
    dev = ctx.fields()
    assert tuple(dev) == NAMES and all(dev[f].shape == (ctx.n,) + SHAPE[f] and dev[f].dtype == F for f in NAMES)
    assert_bits(dev, ref, what + ", host path")
    for f in NAMES:
        assert_bits(ctx.fields(f), {f: ref[f]}, "%s, %s alone" % (what, f))
    for sub in (("divergence", "color_grad"), ("vel_grad", "vorticity")):
        got = ctx.fields(sub)
        assert tuple(got) == sub
        assert_bits(got, {f: ref[f] for f in sub}, "%s, subset %s" % (what, sub))
    if torch_too:
        assert_bits(device_path(ctx), ref, what + ", device-pointer path")
        assert_bits(device_path(ctx, ("color_grad",)), {"color_grad": ref["color_grad"]}, what + ", device-pointer path, colour only")
        assert_bits(device_path(ctx, ("vorticity", "divergence")), {f: ref[f] for f in ("vorticity", "divergence")}, what + ", device-pointer path")
    if bound:
        r64, mag, k = fr.fields64(ctx.params, st, counts, lists)
        r = fr.assert_within_bound(dev, r64, mag, k, what)
        print("%s: bound ratios %s" % (what, r))
    return st, counts, lists, dev


# ----------------------------------------------------------------------------------------------------------------------- bit equality
def test_reference_scene_after_1_and_300_dfsph_steps():
    ctx, timer = scene_ctx(), y.TimeManager()
    assert ctx.n == 4050 and ctx.n % 256 != 0
    dfsph_step(ctx, timer)
    check_state(ctx, "DFSPH step 1")
    for _ in range(299):
        dfsph_step(ctx, timer)
    st, counts, lists, dev = check_state(ctx, "DFSPH step 300")
    assert (counts[:, 1] > counts[:, 0]).any() and dev["vorticity"].any() and dev["divergence"].any()  # walls reached, the flow shears
    # the colour gradient: small in the bulk, of order one at the free surface
    mag = np.sqrt((dev["color_grad"].astype(np.float64) ** 2).sum(1)) * 0.02
    assert np.median(mag) < 0.3 and mag.max() > 0.8


def test_reference_scene_after_30_wcsph_steps():
    ctx, timer = scene_ctx(), y.TimeManager(cfl_factor=0.2)
    for _ in range(30):
        wcsph_step(ctx, timer)
    check_state(ctx, "WCSPH step 30")


@pytest.mark.parametrize("span", [0, y.LISTS_32BIT, 8])
def test_list_formats(span):
    """the window format (16-bit slots of the staged records), the wide format (global slots, gathered from memory) and a mix of both"""
    p = y.default_params()
    p.list_span_limit = span
    ctx, timer = scene_ctx(params=p), y.TimeManager()
    for _ in range(60):
        dfsph_step(ctx, timer)
    st, counts, lists, dev = check_state(ctx, "list_span_limit %#x" % span, torch_too=(span != 0))
    assert (counts[:, 1] > counts[:, 0]).any()
    # the result does not depend on the format
    if span:
        ref_ctx, t2 = scene_ctx(), y.TimeManager()
        for _ in range(60):
            dfsph_step(ref_ctx, t2)
        assert_bits(dev, ref_ctx.fields(), "list_span_limit %#x against the default format" % span)


def test_64800_particles_over_more_than_one_xcd_chunk():
    ctx, timer = scene_ctx(4.0), y.TimeManager()
    assert ctx.n == 64800 and (ctx.n + 255) // 256 == 254
    for _ in range(50):
        _, stats = dfsph_step(ctx, timer)
    assert stats["remote_entries"] > 0  # out-of-window table entries are in use
    check_state(ctx, "dam_break(4.0) step 50")


def test_capped_lists_are_followed():
    pos = (uniform_points(3000, 45000.0, 7) + F(0.4)).astype(F)
    ctx = built_ctx(pos)
    assert ctx.last_flags() & y.FLAG_NEIGHBOR_CAP
    st, counts, lists, dev = check_state(ctx, "capped lists")
    assert counts[:, 1].max() == 64 and (counts[:, 1] == 64).sum() > 10 and (counts[:, 1] < 64).sum() > 10


@pytest.mark.parametrize("n, b", [(1, 0), (2, 0), (63, 0), (1, 8), (63, 200), (257, 64)])
def test_size_edges(n, b):
    """one particle (an empty list: zeros), two, a wavefront less one, and a particle whose only neighbours are boundary particles"""
    pos, bnd = lattice_scene(n, b)
    rng = np.random.default_rng(n * 1000 + b)
    vel = rng.normal(0, 1, pos.shape).astype(F)
    ctx = built_ctx(pos, bnd, vel)
    st, counts, lists, dev = check_state(ctx, "n = %d, b = %d" % (n, b))
    if (n, b) == (1, 0):
        assert counts.tolist() == [[0, 0]] and not any(dev[f].any() for f in NAMES)
    if (n, b) == (1, 8):
        assert counts[0, 0] == 0 and counts[0, 1] > 0 and dev["color_grad"].any() and dev["vel_grad"].any()
    if b and n > 1:
        assert (counts[:, 1] > counts[:, 0]).any() and (counts[:, 0] > 0).any()


def test_lattice_anchor_rotation_and_expansion():
    """the sign and the scale: rigid rotation has vorticity 2 Omega beta and no divergence, uniform expansion divergence 2 a beta and no
    vorticity, beta the lattice's moment factor (float64, from the downloaded lists and densities)"""
    omega, a = 1.5, -0.75
    pos, _ = fr.lattice(32, 0.01)
    x = pos.astype(np.float64)
    for field, which in ((omega * np.stack([-x[:, 1], x[:, 0]], -1), "rotation"), (a * x, "expansion")):
        ctx = built_ctx(pos, None, field.astype(F))
        st, counts, lists, dev = check_state(ctx, "lattice, " + which, torch_too=False)
        K = consts_of(ctx)
        ij = np.rint((st["pos"].astype(np.float64) - 0.5) / 0.01).astype(int)
        idx = np.nonzero(((ij >= 3) & (ij < 29)).all(1))[0]
        assert len(idx) == 26 * 26
        B = np.array([fr.lattice_beta(K, st["pos"], st["density"], i, counts, lists) for i in idx])
        beta = 0.5 * (B[:, 0] + B[:, 1])
        assert (beta > 0.9).all() and (beta < 1.0).all()
        if which == "rotation":
            np.testing.assert_allclose(dev["vorticity"][idx], 2.0 * omega * beta, rtol=1e-4)
            assert np.abs(dev["divergence"][idx] / (2.0 * omega * beta)).max() < 1e-4
        else:
            np.testing.assert_allclose(dev["divergence"][idx], 2.0 * a * beta, rtol=1e-4)
            assert np.abs(dev["vorticity"][idx] / (2.0 * a * beta)).max() < 1e-4


# ----------------------------------------------------------------------------------------------------------------------- state rules
def _rc(ctx, flags=0, out=None):
    d = np.zeros(4 * max(ctx.n, 1), F)
    o = _lib.SphxFieldsOut(divergence=d.ctypes.data) if out is None else out
    return ctx.L.sphx_particle_fields(ctx.h, flags, C.byref(o) if o else None)


def _msg(ctx):
    return ctx.L.sphx_last_error(ctx.h).decode()


def test_state_rules_and_argument_errors():
    R, E = _lib.ERR_NOT_READY, _lib.ERR_INVALID_ARGUMENT
    fresh = y.SphxContext()
    assert _rc(fresh) == R and "no particles uploaded" in _msg(fresh)          # a context in neither state
    ctx = scene_ctx()
    assert _rc(ctx) == R and "sphx_particle_fields" in _msg(ctx)                # after sphx_upload
    ctx.update_neighborhood()
    assert _rc(ctx) == R and "sphx_update_densities" in _msg(ctx)              # a build without densities
    ctx.update_densities(y.KERNEL_WENDLAND_C2)
    assert _rc(ctx) == _lib.OK                                                  # sphx_update_neighborhood + sphx_update_densities
    ctx.set_boundary(ctx.download_boundary()[0])
    assert _rc(ctx) == R and "sphx_set_boundary" in _msg(ctx)                   # after sphx_set_boundary
    timer = y.TimeManager()
    dfsph_step(ctx, timer)
    assert _rc(ctx) == _lib.OK                                                  # after a finished DFSPH step
    ctx.step_begin(timer.simulation_step())
    assert _rc(ctx) == R and "step_begin" in _msg(ctx)                          # between step_begin and step_finish
    ctx.step_finish(y.duration_as_secs_f32(timer.update_simulation_step(DIAM, 0.0)))
    assert _rc(ctx) == _lib.OK
    # argument errors, on a ready context
    assert ctx.L.sphx_particle_fields(None, 0, None) == E                       # ctx NULL
    assert _rc(ctx, out=False) == E and "out is NULL" in _msg(ctx)              # out NULL
    assert _rc(ctx, out=_lib.SphxFieldsOut()) == E and "every pointer is NULL" in _msg(ctx)
    assert _rc(ctx, flags=2) == E and "flags" in _msg(ctx) and _rc(ctx, flags=0x80000001) == E
    for bad in ((), ("density",), "speed"):
        with pytest.raises(ValueError):
            ctx.fields(bad)
    import torch

    with pytest.raises(ValueError):
        ctx.fields(out={"divergence": torch.zeros(ctx.n + 1, device="cuda")})
    # a refused step: the step did not finish
    ctx.step_begin(timer.simulation_step())
    with pytest.raises(y.SphxError):
        ctx.step_finish(-1.0)
    assert _rc(ctx) == R and "run a step" in _msg(ctx)
    dfsph_step(ctx, timer)
    assert _rc(ctx) == _lib.OK
    # sphx_remove / sphx_append: stale once something changed, untouched otherwise
    assert ctx.remove((5.0, 5.0, 6.0, 6.0)) == 0 and _rc(ctx) == _lib.OK
    assert ctx.remove((0.2, 0.4, 0.7, 0.9)) > 0
    assert _rc(ctx) == R
    dfsph_step(ctx, timer)
    assert _rc(ctx) == _lib.OK
    ctx.append(np.array([[1.5, 1.0], [1.52, 1.0]], F))
    assert _rc(ctx) == R
    dfsph_step(ctx, timer)
    assert _rc(ctx) == _lib.OK
    # sphx_state_load: of a ready state ready (and the same bits), of a state that was not ready not
    want = ctx.fields()
    blob = ctx.save_state()
    other = y.SphxContext()
    other.load_state(blob)
    assert_bits(other.fields(), want, "after sphx_state_load into a fresh context")
    ctx.upload(dam_break(1.0)[0])
    assert _rc(ctx) == R
    other.load_state(ctx.save_state())
    assert _rc(other) == R
    # WCSPH: after a step, and between its two phases
    w, t = scene_ctx(), y.TimeManager(cfl_factor=0.2)
    wcsph_step(w, t)
    assert _rc(w) == _lib.OK
    w.wcsph_step_begin(t.simulation_step())
    assert _rc(w) == R and "step_begin" in _msg(w)
    # a tile context is refused as an argument
    tc = scene_ctx()
    assert tc.L.sphx_tile_configure(tc.h, 0, 0, 65536, 4, 0, 0) == _lib.OK
    assert _rc(tc) == E and "tile" in _msg(tc)


def test_zero_fluid_particles():
    """A step over zero fluid particles runs no neighbour build: not ready.  n == 0 in a ready context: a successful no-op."""
    _, bnd = dam_break(1.0)
    for wcsph in (False, True):
        ctx = y.SphxContext()
        ctx.set_boundary(bnd)
        ctx.upload(np.zeros((0, 2), F))
        t = y.TimeManager(cfl_factor=0.2) if wcsph else y.TimeManager()
        (wcsph_step if wcsph else dfsph_step)(ctx, t)
        assert _rc(ctx) == _lib.ERR_NOT_READY and "sphx_update_neighborhood" in _msg(ctx)
        ctx.update_neighborhood()
        ctx.update_densities(y.KERNEL_WENDLAND_C2)
        assert _rc(ctx) == _lib.OK and _rc(ctx, flags=_lib.FIELDS_DEVICE_POINTERS) == _lib.OK
        out = ctx.fields()
        assert out["vel_grad"].shape == (0, 2, 2) and out["color_grad"].shape == (0, 2)


# ----------------------------------------------------------------------------------------------------------------------- side effects
def _run(n_steps, calls, wcsph, run_ahead, monkeypatch):
    monkeypatch.setenv("SPHX_RUN_AHEAD", "1" if run_ahead else "0")
    ctx = scene_ctx()
    timer = y.TimeManager(cfl_factor=0.2) if wcsph else y.TimeManager()
    log = []
    if calls:
        import torch

        dev_out = {"vel_grad": torch.zeros((ctx.n, 2, 2), device="cuda"), "color_grad": torch.zeros((ctx.n, 2), device="cuda")}
    for s in range(n_steps):
        vmax, st = (wcsph_step if wcsph else dfsph_step)(ctx, timer)
        log.append((F(vmax), timer.simulation_step_ns(), tuple(sorted(st.items())), ctx.last_flags()))
        if calls:
            ctx.fields()
            ctx.fields("color_grad")
            ctx.fields(out=dev_out)
            assert ctx.last_flags() == log[-1][3]
    return log, ctx.state_digest(), ctx.download()


@pytest.mark.parametrize("wcsph, steps", [(False, 60), (True, 30)])
@pytest.mark.parametrize("run_ahead", [True, False])
def test_calls_have_no_side_effects(wcsph, steps, run_ahead, monkeypatch):
    log_a, dig_a, a = _run(steps, False, wcsph, run_ahead, monkeypatch)
    log_b, dig_b, b = _run(steps, True, wcsph, run_ahead, monkeypatch)
    assert log_b == log_a, "step stats, vmax, the timer's step or sphx_last_flags differ"
    assert dig_a == dig_b and len(dig_a) == 9
    for k in ("pos", "vel", "density", "ids"):
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k


# ----------------------------------------------------------------------------------------------------------------------- harness
def test_harness_fields_csv_equals_the_python_call(tmp_path):
    steps = 80  # (the column has reached the floor: the flow shears)
    path = tmp_path / "fields.csv"
    out = subprocess.run([HARNESS, "--scale", "1", "--steps", str(steps), "--warmup", "0", "--fields-out", str(path)], capture_output=True, text=True,
                         timeout=600)
    assert out.returncode == 0, out.stderr
    assert '"fields_particles": 4050' in out.stdout
    lines = path.read_text().splitlines()
    assert lines[0] == "id,x,y,divergence,vorticity,cx,cy" and len(lines) == 1 + 4050
    csv = np.array([[float(v) for v in ln.split(",")] for ln in lines[1:]])
    w = y.FluidParticleWorld()
    w.reset_fluid(1.0)
    ctx = y.SphxContext()
    ctx.set_boundary(w.boundary_particles)
    ctx.upload(w.positions)
    timer = y.TimeManager()
    for _ in range(steps):
        timer.on_step_started()  # the harness advances the clock like simulation_frame_loop does (timemanager.rs:244-247)
        dfsph_step(ctx, timer)
    d, f = ctx.download(), ctx.fields()
    assert np.array_equal(csv[:, 0].astype(np.uint32), d["ids"])
    assert_bits({"pos": csv[:, 1:3].astype(F), "divergence": csv[:, 3].astype(F), "vorticity": csv[:, 4].astype(F), "color_grad": csv[:, 5:7].astype(F)},
                {"pos": d["pos"], "divergence": f["divergence"], "vorticity": f["vorticity"], "color_grad": f["color_grad"]}, "--fields-out")
    assert f["vorticity"].any()
    bad = subprocess.run([HARNESS, "--scale", "1", "--steps", "1", "--warmup", "0", "--fields-out"], capture_output=True, text=True, timeout=120)
    assert bad.returncode == 2
