"""sphx_append / sphx_remove without a GPU: the numpy restatement of the contract (tests/edit_reference.py — what the GPU tests compare
the device with) on hand cases, the header, the exports and the bindings of the four functions, their NULL handling, the harness
options, and the oracle's behaviour on the scenes tests/test_gpu_edit.py runs (finite, no neighbour flags, the removal counts)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import edit_reference as ref
import yasph2d_amd as y
from oracle.oracle import Oracle
from yasph2d_amd import _lib

F = np.float32
INF = float("inf")
NAN = float("nan")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "yasph2d_amd", "sphx_harness")
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "dam_break_4050.npz"))


# ---- the reference's own hand cases -------------------------------------------------------------------------------------------------
def test_predicate_is_half_open_on_every_bound():
    r = (1.0, 2.0, 3.0, 4.0)
    below = np.nextafter(F(3.0), F(0.0))
    pts = [(1.0, 2.0), (3.0, 2.0), (1.0, 4.0), (below, 2.0), (1.0, np.nextafter(F(4.0), F(0.0))), (np.nextafter(F(1.0), F(0.0)), 3.0),
           (2.0, np.nextafter(F(2.0), F(0.0))), (2.0, 3.0)]
    assert ref.in_rect(r, pts).tolist() == [True, False, False, True, True, False, False, True]


def test_predicate_special_values():
    denorm = np.float32(1e-45)
    pts = np.array([(0.0, 0.0), (-0.0, -0.0), (denorm, denorm), (-denorm, 0.0), (NAN, 0.5), (0.5, NAN), (INF, 0.5), (-INF, 0.5)], F)
    # [0, 1) x [0, 1): -0 == +0 is inside, a negative denormal is not, NaN and the infinities are in no finite rectangle
    assert ref.removed_mask(pts, (0.0, 0.0, 1.0, 1.0)).tolist() == [True, True, True, False, False, False, False, False]
    # the whole plane holds everything but NaN (+inf fails x < +inf)
    assert ref.removed_mask(pts, (-INF, -INF, INF, INF)).tolist() == [True, True, True, True, False, False, False, True]
    # OUTSIDE is the complement: a keep-box drops NaN particles
    assert ref.removed_mask(pts, (-INF, -INF, INF, INF), outside=True).tolist() == [False, False, False, False, True, True, True, False]
    # half planes
    assert ref.removed_mask(pts, (0.0, -INF, INF, INF)).tolist() == [True, True, True, False, False, False, False, False]
    # x0 > x1 is empty; no rectangle removes nothing, or everything with OUTSIDE
    assert not ref.removed_mask(pts, (1.0, 0.0, 0.0, 1.0)).any()
    assert not ref.removed_mask(pts, []).any() and ref.removed_mask(pts, [], outside=True).all()


def test_overlapping_rectangles_remove_once_and_limits_are_refused():
    pts = np.array([(0.5, 0.5), (1.5, 0.5), (2.5, 0.5)], F)
    rects = [(0.0, 0.0, 2.0, 1.0), (1.0, 0.0, 2.0, 1.0)]
    pos, vel, ids, removed = ref.remove(pts, pts * 2, np.array([7, 8, 9], np.uint32), rects)
    assert removed == 2 and pos.tolist() == [[2.5, 0.5]] and vel.tolist() == [[5.0, 1.0]] and ids.tolist() == [9]
    with pytest.raises(ValueError):
        ref.as_rects([(0.0, 0.0, 1.0, 1.0)] * 9)
    with pytest.raises(ValueError):
        ref.as_rects((0.0, NAN, 1.0, 1.0))
    assert ref.as_rects([(0.0, 0.0, 1.0, 1.0)] * 8).shape == (8, 4)


def test_filter_keeps_order_and_append_numbers_from_first_id():
    pos = np.stack([np.where(np.arange(10) % 3 == 0, 0.75, 0.25), np.arange(10) / 16.0], -1).astype(F)
    vel = np.stack([np.arange(10), -np.arange(10)], -1).astype(F)
    ids = np.arange(10, dtype=np.uint32)[::-1].copy()
    p, v, i, removed = ref.remove(pos, vel, ids, (0.5, -INF, 1.0, INF))
    assert removed == 4 and i.tolist() == [8, 7, 5, 4, 2, 1] and v[:, 0].tolist() == [1, 2, 4, 5, 7, 8]
    p2, v2, i2 = ref.append(p, v, i, [(9.0, 9.0), (8.0, 8.0)], None, 10)
    assert len(p2) == 8 and i2.tolist() == [8, 7, 5, 4, 2, 1, 10, 11] and v2[6:].tolist() == [[0, 0], [0, 0]] and p2[7].tolist() == [8.0, 8.0]
    assert ref.append(p, v, i, np.zeros((1, 2)), [(1.0, 2.0)], 0xFFFFFFFF)[2][-1] == 0xFFFFFFFF


# ---- header, exports, bindings ------------------------------------------------------------------------------------------------------
EDIT_FUNCTIONS = ("sphx_append", "sphx_remove", "sphx_solver_append", "sphx_solver_remove")


def test_header_declares_the_edit_calls_under_abi_5():
    src = open(os.path.join(ROOT, "include", "sphx.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for fn in EDIT_FUNCTIONS:
        assert re.search(r"\bint %s\s*\(" % fn, code), fn
    assert re.search(r"typedef struct sphx_rect \{ float x0, y0, x1, y1; \} sphx_rect;", code)
    assert re.search(r"#define SPHX_REMOVE_MAX_RECTS 8\b", code) and re.search(r"SPHX_REMOVE_OUTSIDE = 1u", code)
    assert re.search(r"#define SPHX_ABI_VERSION 5\b", code)
    assert "5 (additive): sphx_append, sphx_remove" in src


def test_edit_symbols_exported_bound_and_null_ctx_rejected(sphx_lib):
    for fn in EDIT_FUNCTIONS:
        assert hasattr(sphx_lib, fn) and fn in _lib.SIGNATURES, fn
    assert C.sizeof(_lib.SphxRect) == 16 and (_lib.REMOVE_OUTSIDE, _lib.REMOVE_MAX_RECTS) == (1, ref.MAX_RECTS)
    r = _lib.SphxRect(0.0, 0.0, 1.0, 1.0)
    out = C.c_uint32(77)
    xy = np.zeros((1, 2), F)
    assert sphx_lib.sphx_remove(None, C.byref(r), 1, 0, C.byref(out)) == _lib.ERR_INVALID_ARGUMENT
    assert sphx_lib.sphx_append(None, xy.ctypes.data, None, 1, C.byref(out)) == _lib.ERR_INVALID_ARGUMENT
    assert sphx_lib.sphx_solver_remove(None, None, C.byref(r), 1, 0, 1, C.byref(out)) == _lib.ERR_INVALID_ARGUMENT
    assert sphx_lib.sphx_solver_append(None, None, xy.ctypes.data, None, 1, 1, C.byref(out)) == _lib.ERR_INVALID_ARGUMENT
    assert out.value == 77


def test_python_rectangle_arguments():
    arr, k = y._rect_array((0.0, 1.0, 2.0, INF))
    assert k == 1 and (arr[0].x0, arr[0].y0, arr[0].x1, arr[0].y1) == (0.0, 1.0, 2.0, INF)
    arr, k = y._rect_array([(0, 0, 1, 1), (-INF, 2, 3, 4)])
    assert k == 2 and arr[1].x0 == -INF and arr[1].y1 == 4.0
    assert y._rect_array([]) == (None, 0)
    with pytest.raises(ValueError):
        y._rect_array([(0, 0, 1)])
    with pytest.raises(ValueError):
        y._append_arrays(np.zeros((3, 2)), np.zeros((2, 2)))


@pytest.mark.parametrize("args", [["--drain", "0,0,1"], ["--keep", "0,0,1,nan"], ["--emit", "0,0,1"], ["--emit", "0,0,1,1:every=0"],
                                  ["--emit", "0,0,1,1:speed=3"], ["--emit", "0,0,inf,1"],
                                  sum((["--drain", "0,0,1,1"] for _ in range(5)), []) + sum((["--keep", "0,0,1,inf"] for _ in range(4)), [])])
def test_harness_rejects_bad_edit_options(sphx_lib, args):
    """(argument errors end the harness before it touches a device)"""
    out = subprocess.run([HARNESS] + args, capture_output=True, text=True, timeout=60)
    assert out.returncode == 2, (out.returncode, out.stderr)
    assert "invalid --" in out.stderr


# ---- the oracle on the scenes of tests/test_gpu_edit.py ------------------------------------------------------------------------------
def oracle_after(steps):
    o = Oracle()
    o.set_boundary(GOLD["in_boundary"])
    o.set_particles(GOLD["in_pos"])
    for _ in range(steps):
        o.dfsph_step()
    return o


def oracle_remove(o, rects, outside=False):
    p, v = o.positions(), o.velocities()
    gone = ref.removed_mask(p, rects, outside)
    o.set_particles(p[~gone], v[~gone])
    return int(gone.sum())


def run_clean(o, steps):
    flags = 0
    stats = []
    for _ in range(steps):
        stats.append(o.dfsph_step())
        flags |= stats[-1]["neighbor_flags"]
    assert flags == 0
    assert np.isfinite(o.positions()).all() and np.isfinite(o.velocities()).all() and np.isfinite(o.densities()).all()
    return stats


def test_oracle_stays_clean_on_the_removal_cases_after_150_steps():
    """One 150-step run, the five removals counted on it; the first is also run on."""
    o = oracle_after(150)
    p = o.positions()
    counts = [int(ref.removed_mask(p, r, out).sum()) for r, out in (
        ([(0.6, -INF, INF, INF)], False), ([(0.2, 0.4, 0.7, 0.9)], False), ([(-INF, -INF, INF, 0.7)], False),
        ([(0, 1, 0.3, INF), (0.6, -INF, INF, 0.8)], False), ([(0, 0.5, 0.7, 1.3)], True))]
    assert counts == [200, 1415, 845, 874, 505]
    assert oracle_remove(o, (0.6, -INF, INF, INF)) == 200
    run_clean(o, 40)


def test_oracle_stays_clean_after_600_steps_with_the_divergence_warm_start_firing():
    o = oracle_after(600)
    assert int(ref.removed_mask(o.positions(), (0, 0, 1.5, 2.5), True).sum()) == 1037
    assert oracle_remove(o, (1.0, -INF, INF, INF)) == 1665
    stats = run_clean(o, 60)
    assert sum(s["divergence_iterations"] == 2 and s["warmstart_divergence"] == 1 for s in stats) == 60


def test_oracle_wcsph_stays_finite_on_the_wcsph_case():
    """600 WCSPH steps bring 195 particles past x = 0.6 (no step of this run has exactly 200 there)."""
    t = y.TimeManager(cfl_factor=0.2)
    o = Oracle()
    o.timer_adaptive(t.timestep_max_ns, t.timestep_min_ns, 0.2)
    o.set_boundary(GOLD["in_boundary"])
    o.set_particles(GOLD["in_pos"])
    for _ in range(600):
        o.wcsph_step()
    assert oracle_remove(o, (0.6, -INF, INF, INF)) == 195
    for _ in range(30):
        o.wcsph_step()
    assert np.isfinite(o.positions()).all() and np.isfinite(o.velocities()).all() and np.isfinite(o.densities()).all()
