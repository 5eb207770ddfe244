"""Per-particle flow fields without a GPU: the C ABI exports the call and checks its context argument; the float32 restatement of the
contract (tests/fields_reference.py), which the GPU tests compare the device with bit for bit, is itself checked against hand-made
cases, the float64 sums over the oracle's neighbour lists and densities, and the analytic gradient of linear velocity fields."""
import ctypes as C

import numpy as np
import pytest

import fields_reference as fr
import sample_reference as sr
import yasph2d_amd as y
from util import dam_break
from yasph2d_amd import _lib

F = np.float32


def test_fields_symbol_exported_and_null_context_rejected(sphx_lib):
    assert hasattr(sphx_lib, "sphx_particle_fields") and "sphx_particle_fields" in _lib.SIGNATURES
    d = np.zeros(4, np.float32)
    out = _lib.SphxFieldsOut(divergence=d.ctypes.data)
    assert sphx_lib.sphx_particle_fields(None, 0, C.byref(out)) == _lib.ERR_INVALID_ARGUMENT
    assert sphx_lib.sphx_particle_fields(None, 0, None) == _lib.ERR_INVALID_ARGUMENT
    assert y.FIELD_NAMES == fr.NAMES and _lib.FIELDS_DEVICE_POINTERS == 1
    assert C.sizeof(_lib.SphxFieldsOut) == 4 * C.sizeof(C.c_void_p)
    assert hasattr(y.SphxContext, "fields")


def _consts():
    return fr.Constants(y.default_params())


def _state(pos, vel, rho, bnd=None):
    return dict(pos=np.asarray(pos, F).reshape(-1, 2), vel=np.asarray(vel, F).reshape(-1, 2), density=np.asarray(rho, F),
                boundary=np.zeros((0, 2), F) if bnd is None else np.asarray(bnd, F).reshape(-1, 2))


def test_constants_follow_sphx_create():
    K = _consts()
    assert K.w_hinv == F(F(1.0) / F(0.02)) and K.mass == F(0.01) and K.rho0 == F(100.0)
    assert float(K.w_ngrad) == pytest.approx(140.0 / (np.pi * float(K.h) ** 4), rel=1e-6)


def test_single_particle_gives_zeros():
    K = _consts()
    st = _state([[0.5, 0.5]], [[0.3, -1.0]], [100.0])
    counts, lists = fr.host_neighbours(K, st["pos"])
    assert counts.tolist() == [[0, 0]] and len(lists) == 0
    out = fr.fields32(K, st, counts, lists)
    for k in fr.NAMES:
        assert out[k].dtype == F and not out[k].any(), k
    assert out["vel_grad"].shape == (1, 2, 2) and out["color_grad"].shape == (1, 2)
    # no particles at all
    e = fr.fields32(K, _state(np.zeros((0, 2)), np.zeros((0, 2)), []), np.zeros((0, 2), np.uint16), np.zeros(0, np.uint32))
    assert e["vel_grad"].shape == (0, 2, 2) and e["divergence"].shape == (0,)


def test_two_particles_antisymmetric_colour_gradient_and_the_expressions():
    K = _consts()
    p = np.array([[0.25, 0.75], [0.25 + 2.0 ** -7, 0.75 - 2.0 ** -8]], F)  # (exact in fp32: d and -d)
    v = np.array([[1.0, 2.0], [-0.5, 0.25]], F)
    st = _state(p, v, [100.0, 100.0])
    counts, lists = fr.host_neighbours(K, p)
    assert counts.tolist() == [[1, 1], [1, 1]] and lists.tolist() == [1, 0]
    out = fr.fields32(K, st, counts, lists)
    cg = out["color_grad"]
    assert (cg[0] == -cg[1]).all() and cg[0, 0] > 0 and cg[0, 1] < 0  # towards the neighbour
    # the contract, scalar by scalar, for particle 0
    dx, dy = F(p[1, 0] - p[0, 0]), F(p[1, 1] - p[0, 1])
    r = np.sqrt(F(F(dx * dx) + F(dy * dy)))
    omq = F(F(1.0) - min(F(r * K.w_hinv), F(1.0)))
    s = F(F(F(K.w_ngrad * omq) * omq) * omq)
    vol = F(K.mass / F(100.0))
    ax, ay = F(vol * F(s * dx)), F(vol * F(s * dy))
    dvx, dvy = F(v[1, 0] - v[0, 0]), F(v[1, 1] - v[0, 1])
    want = np.array([[F(dvx * ax), F(dvx * ay)], [F(dvy * ax), F(dvy * ay)]], F)
    assert (out["vel_grad"][0] == want).all() and (cg[0] == np.array([ax, ay], F)).all()
    assert out["divergence"][0] == F(want[0, 0] + want[1, 1]) and out["vorticity"][0] == F(want[1, 0] - want[0, 1])
    # a static neighbour: volume m / rho0, velocity zero
    st_b = _state(p[:1], v[:1], [123.0], bnd=p[1:])
    cb, lb = fr.host_neighbours(K, p[:1], p[1:])
    assert cb.tolist() == [[0, 1]] and lb.tolist() == [0]
    ob = fr.fields32(K, st_b, cb, lb)
    vb = F(K.mass / K.rho0)
    axb = F(vb * F(s * dx))
    assert ob["color_grad"][0, 0] == axb and ob["vel_grad"][0, 0, 0] == F(F(F(0.0) - v[0, 0]) * axb)


def _oracle_state(steps, wcsph=False):
    from oracle.oracle import Oracle

    pos, boundary = dam_break(1.0)
    o = Oracle()
    if wcsph:
        t = y.TimeManager(cfl_factor=0.2)
        o.timer_adaptive(t.timestep_max_ns, t.timestep_min_ns, 0.2)
    o.set_boundary(boundary)
    o.set_particles(pos)
    for _ in range(steps):
        o.wcsph_step() if wcsph else o.dfsph_step()
    st = dict(pos=o.positions(), vel=o.velocities(), density=o.densities(), boundary=o.boundary())
    counts, _, lists = o.neighbors()
    return st, counts, lists


@pytest.mark.parametrize("steps, wcsph", [(1, False), (60, False), (300, False), (30, True)])
def test_restatement_within_float64_bound_on_oracle_states(steps, wcsph):
    st, counts, lists = _oracle_state(steps, wcsph)
    K = _consts()
    params = y.default_params()
    dev = fr.fields32(K, st, counts, lists)
    ref, mag, k = fr.fields64(params, st, counts, lists)
    r = fr.assert_within_bound(dev, ref, mag, k, "steps %d wcsph %s" % (steps, wcsph))
    print("bound ratios after %d steps (wcsph %s): %s" % (steps, wcsph, r))
    assert max(r.values()) < 0.5, r
    # guard: a slip of the contract lands far beyond the bound — the boundary neighbours left out, vel_grad transposed.  A state shows a
    # slip once the fluid has reached a wall resp. the flow shears (after one DFSPH step or 30 WCSPH steps the column is still in free
    # fall, away from the walls: both slips change nothing there); the 60- and 300-step states show both.
    no_b = fr.bound_ratios(fr.fields32(K, st, counts, lists, boundary_neighbours=False), ref, mag, k)
    tr = fr.bound_ratios(dict(vel_grad=dev["vel_grad"].transpose(0, 2, 1)), ref, mag, k)
    print("guard ratios: boundary left out %s, transposed %s" % (no_b, tr))
    at_wall = bool((counts[:, 1] > counts[:, 0]).any())
    shears = bool((ref["vel_grad"] != ref["vel_grad"].transpose(0, 2, 1)).any())
    if not wcsph and steps >= 60:
        assert at_wall and shears
    if at_wall:
        assert no_b["color_grad"] > 100 and no_b["vel_grad"] > 100
    if shears:
        assert tr["vel_grad"] > 100


def test_colour_gradient_marks_the_free_surface():
    """|color_grad| h: small in the bulk of the settled column, of order one at its surface (no threshold is built in)."""
    st, counts, lists = _oracle_state(1)
    K = _consts()
    cg = fr.fields32(K, st, counts, lists)["color_grad"].astype(np.float64)
    mag = np.sqrt((cg * cg).sum(1)) * float(K.h)
    pos = st["pos"]
    top = pos[:, 1] >= pos[:, 1].max() - 1e-4
    assert np.median(mag) < 0.2 and mag[top].min() > 0.5
    assert (cg[top, 1] < 0).all()  # into the fluid: downwards at the top row


def _lattice_state(field):
    K = _consts()
    pos, inner = fr.lattice(32, 0.01)
    counts, lists = fr.host_neighbours(K, pos)
    rho = fr.wendland_density(K, pos, counts, lists, sr.Constants(y.default_params()).w_norm)
    vel = field(pos.astype(np.float64)).astype(F)
    return K, _state(pos, vel, rho), counts, lists, inner


def lattice_expectations(K, st, counts, lists, inner):
    """beta = (Bxx + Byy) / 2 of every interior particle (float64) and the largest |Bxy| / beta among them."""
    idx = np.nonzero(inner)[0]
    B = np.array([fr.lattice_beta(K, st["pos"], st["density"], i, counts, lists) for i in idx])
    beta = 0.5 * (B[:, 0] + B[:, 1])
    return idx, beta, float(np.abs(B[:, 2] / beta).max()), float(np.abs((B[:, 0] - B[:, 1]) / beta).max())


def test_lattice_anchor_rotation_and_expansion():
    omega, a = 1.5, -0.75
    K, st, counts, lists, inner = _lattice_state(lambda x: omega * np.stack([-x[:, 1], x[:, 0]], -1))
    idx, beta, cross, aniso = lattice_expectations(K, st, counts, lists, inner)
    assert (beta > 0.9).all() and (beta < 1.0).all() and cross < 1e-5 and aniso < 1e-5, (beta.min(), beta.max(), cross, aniso)
    assert beta[0] == pytest.approx(0.9409, abs=2e-3)
    out = fr.fields32(K, st, counts, lists)
    scale = 2.0 * omega * beta
    np.testing.assert_allclose(out["vorticity"][idx], scale, rtol=1e-4)
    assert np.abs(out["divergence"][idx] / scale).max() < 1e-4
    assert np.abs(out["color_grad"][idx]).max() * float(K.h) < 1e-3  # the bulk: no colour gradient
    K, st, counts, lists, inner = _lattice_state(lambda x: a * x)
    out = fr.fields32(K, st, counts, lists)
    scale = 2.0 * a * beta
    np.testing.assert_allclose(out["divergence"][idx], scale, rtol=1e-4)
    assert np.abs(out["vorticity"][idx] / scale).max() < 1e-4
