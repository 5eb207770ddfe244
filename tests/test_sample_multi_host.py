"""Sampling the fields of a tiled run (sphx_multi_sample_points / _grid, include/sphx.h), the parts that need no GPU: the lattice
window of a tile and the fold of the ranks' parts as a sanitized stand-alone program, the window against the numpy restatement of the
cell function, the exported fold through the bindings against a numpy restatement, and the exports / bindings / NULL handling."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import yasph2d_amd as ya
from sample_reference import cells_of, lattice_points
from yasph2d_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "yasph2d_amd", "csrc")
F = np.float32
MULTI_CALLS = ("sphx_multi_sample_points", "sphx_multi_sample_grid", "sphx_sample_merge", "sphx_multi_tile_rects", "sphx_multi_ghost_rings")
TILE_CALLS = ("sphx_tile_sample_points", "sphx_tile_sample_points_fetch", "sphx_tile_sample_window", "sphx_tile_sample_window_fetch")


# ------------------------------------------------------------------------------------------------------ 1. the window header, sanitized
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to compile the sample-window driver"
    exe = str(tmp_path_factory.mktemp("sample_window") / "sample_window_driver")
    # -ffp-contract=off: a fused x0 + ix * dx is a different point (the library is built with the same flag)
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(ROOT, "tests", "sample_window_driver.cpp"), "-o", exe])

    def run(*args):
        r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
        return r.returncode, r.stdout, r.stderr

    return run


@pytest.mark.parametrize("check", ["check", "merge"])
def test_sample_window_host(driver, check):
    """check: for 480 seeded lattices and rectangles (dx below, equal to and above a cell, nx or ny equal to 1, origins outside the
    domain on either side, spacings whose (float)ix * dx reaches infinity, rectangles touching cell 0 and cell 65536) the bisection's
    index rectangle equals the brute-force set, and three complementary strips partition the lattice.  merge: the fold of the parts
    against a restatement, with out aliasing parts[0], zero parts, unanswered points and points two parts answer.  The sanitizers stay
    clean (any report aborts the program)."""
    rc, out, err = driver(check)
    assert rc == 0 and out.startswith("ok ") and err == "", (out[-2000:], err[-2000:])
    assert int(out.split()[1]) >= (480 if check == "check" else 60)


class _Grid:
    def __init__(self, gx, gy, cell_inv):
        self.gmin, self.cell_inv = np.array([gx, gy], F), F(cell_inv)


def test_window_against_the_numpy_cell_function(driver):
    """A sample of the driver's cases, restated: the window the C++ bisection found is the set of lattice indices whose
    sample_reference.cells_of(lattice_points(...)) lies in the rectangle."""
    rc, out, err = driver("dump", 64)
    assert rc == 0 and err == "", err[-2000:]
    lines = out.strip().splitlines()
    assert len(lines) == 64
    nonempty = 0
    for line in lines:
        w = line.split()
        x0, y0, dx, dy = (np.array([int(v, 16)], np.uint32).view(F)[0] for v in w[:4])
        nx, ny = int(w[4]), int(w[5])
        gx, gy, cell_inv = (np.array([int(v, 16)], np.uint32).view(F)[0] for v in w[6:9])
        cx0, cx1, cy0, cy1, ix0, ix1, iy0, iy1 = (int(v) for v in w[9:])
        with np.errstate(over="ignore"):
            cells = cells_of(_Grid(gx, gy, cell_inv), lattice_points(x0, y0, dx, dy, nx, ny)).reshape(ny, nx, 2)
        inside = (cells[..., 0] >= cx0) & (cells[..., 0] < cx1) & (cells[..., 1] >= cy0) & (cells[..., 1] < cy1)
        want = np.zeros((ny, nx), bool)
        want[iy0:iy1, ix0:ix1] = True
        assert np.array_equal(inside, want), line
        nonempty += bool(inside.any())
    assert nonempty >= 16


def test_window_header_has_no_hip():
    src = open(os.path.join(CSRC, "sphx_sample_window.hpp")).read()
    assert "hip" not in "".join(re.findall(r"#include\s*[<\"]([^>\"]+)", src)).lower()


# ------------------------------------------------------------------------------------------------------ 2. the exported fold
def words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def random_part(rng, shape, tile, p_answered):
    on = rng.random(shape) < p_answered
    part = dict(tile=np.where(on, tile, -1).astype(np.int32))
    for f in ya.SAMPLE_FIELDS:
        full = shape + ((2,) if f == "velocity" else ())
        v = rng.integers(0, 2**32, full, dtype=np.uint64).astype(np.uint32)
        v[~on] = 0
        part[f] = v if f == "count" else v.view(F)
    return part


def merge_reference(parts):
    shape = parts[0]["tile"].shape
    out = {f: np.zeros_like(words(parts[0][f])) for f in ya.SAMPLE_FIELDS}
    tile = np.full(shape, -1, np.int32)
    for p in parts:
        take = (p["tile"] >= 0) & ((tile < 0) | (p["tile"] < tile))
        tile[take] = p["tile"][take]
        for f in out:
            out[f][take] = words(p[f])[take]
    out["tile"] = tile
    return out


def test_exported_merge_against_numpy(sphx_lib):
    rng = np.random.default_rng(21)
    for shape, tiles in (((0,), (0, 1)), ((1,), (3,)), ((257,), (1, 0)), ((1000,), (4, 2, 2, 0, 1)), ((17, 17), (1, 0, 2))):
        parts = [random_part(rng, shape, t, 0.45) for t in tiles]
        want = merge_reference(parts)
        got = ya.sample_merge(parts)
        assert sorted(got) == sorted(want)
        for f in want:
            assert np.array_equal(words(got[f]), words(want[f])), (shape, f)
        if np.prod(shape) > 100:  # (the cases hold a point no part answers and one two parts answer)
            answered = np.sum([p["tile"] >= 0 for p in parts], 0)
            assert (answered == 0).any() and (answered >= 2).any()
            assert (got["tile"][answered == 0] == -1).all() and not words(got["density"])[answered == 0].any()
        # a subset of the fields gives the same bits
        sub = ya.sample_merge([{f: p[f] for f in ("tile", "velocity")} for p in parts])
        assert sorted(sub) == ["tile", "velocity"] and np.array_equal(words(sub["velocity"]), words(want["velocity"]))


def _struct(part):
    o = _lib.SphxMultiSampleOut()
    for f, a in part.items():
        setattr(o, f, a.ctypes.data)
    return o


def test_exported_merge_aliasing_and_zero_parts(sphx_lib):
    L = sphx_lib
    rng = np.random.default_rng(22)
    m = 300
    parts = [random_part(rng, (m,), t, 0.5) for t in (2, 0, 1)]
    want = merge_reference(parts)
    arr = (_lib.SphxMultiSampleOut * 3)(*[_struct(p) for p in parts])
    assert L.sphx_sample_merge(m, arr, 3, C.byref(arr[0])) == 0  # out = parts[0]
    for f in want:
        assert np.array_equal(words(parts[0][f]), words(want[f])), f
    # zero parts: the all-absent answer
    out = random_part(rng, (m,), 5, 1.0)
    assert L.sphx_sample_merge(m, None, 0, C.byref(_struct(out))) == 0
    assert (out["tile"] == -1).all() and not any(words(out[f]).any() for f in ya.SAMPLE_FIELDS)
    # two parts answering one point: the lowest tile wins, whatever the order of the parts
    a, b = random_part(rng, (4,), 3, 1.0), random_part(rng, (4,), 1, 1.0)
    for order in ((a, b), (b, a)):
        got = ya.sample_merge(order)
        assert (got["tile"] == 1).all() and np.array_equal(words(got["fraction"]), words(b["fraction"]))


# ------------------------------------------------------------------------------------------------------ 3. exports, bindings, NULL
def test_header_declares_and_library_exports(sphx_lib):
    full = open(os.path.join(ROOT, "include", "sphx.h")).read()
    src = re.sub(r"/\*.*?\*/", "", full, flags=re.S)
    for name in MULTI_CALLS + TILE_CALLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, src), f"{name} is not declared in include/sphx.h"
        assert hasattr(sphx_lib, name), f"{name} is not exported by libsphx.so"
        assert name in _lib.SIGNATURES
    assert sphx_lib.sphx_abi_version() == 5
    assert "SPHX_ABI_VERSION 5" in src and re.search(r"5 \(additive\): sphx_multi_sample_points", full)
    assert "sampling the fields of a tiled run" in full
    assert C.sizeof(_lib.SphxMultiSampleOut) == 5 * C.sizeof(C.c_void_p)
    from yasph2d_amd.multi import MultiSolver

    for name in ("sample", "sample_grid", "tile_rects", "ghost_rings"):
        assert callable(getattr(MultiSolver, name))
    assert callable(ya.DFSPHMultiSolver.sample) and callable(ya.DFSPHMultiSolver.sample_grid) and "sample_merge" in ya.__all__


def test_null_and_bad_arguments_are_refused(sphx_lib):
    L, bad = sphx_lib, _lib.ERR_INVALID_ARGUMENT
    xy = (C.c_float * 8)()
    buf = (C.c_float * 16)()
    til = (C.c_int32 * 4)()
    o = _lib.SphxMultiSampleOut(C.addressof(buf), None, None, None, C.addressof(til))
    n = C.c_uint32(4)
    rings = (C.c_double * 3)()
    win = (C.c_uint32 * 4)()
    assert L.sphx_multi_sample_points(None, xy, 4, 0, 0, C.byref(o)) == bad
    assert L.sphx_multi_sample_grid(None, 0.0, 0.0, 0.1, 0.1, 2, 2, 0, 0, C.byref(o)) == bad
    assert L.sphx_multi_tile_rects(None, None, C.byref(n)) == bad
    assert L.sphx_multi_ghost_rings(None, rings) == bad
    assert L.sphx_tile_sample_points(None, xy, 4, 0, 1) == bad
    assert L.sphx_tile_sample_points_fetch(None, None, 0, C.byref(n)) == bad
    assert L.sphx_tile_sample_window(None, 0.0, 0.0, 0.1, 0.1, 2, 2, 0, 1, win) == bad
    assert L.sphx_tile_sample_window_fetch(None, None) == bad
    # the fold: out NULL, out requesting nothing, parts NULL with n_parts > 0, a part without tile, out asking for an array a part lacks
    part = _lib.SphxMultiSampleOut(C.addressof(buf), None, None, None, C.addressof(til))
    assert L.sphx_sample_merge(4, C.byref(part), 1, None) == bad
    assert b"out is NULL" in L.sphx_multi_last_error(None)
    assert L.sphx_sample_merge(4, C.byref(part), 1, C.byref(_lib.SphxMultiSampleOut())) == bad
    assert L.sphx_sample_merge(4, None, 1, C.byref(o)) == bad
    no_tile = _lib.SphxMultiSampleOut(C.addressof(buf), None, None, None, None)
    assert L.sphx_sample_merge(4, C.byref(no_tile), 1, C.byref(o)) == bad
    assert b"tile" in L.sphx_multi_last_error(None)
    wants_fraction = _lib.SphxMultiSampleOut(None, C.addressof(buf), None, None, C.addressof(til))
    assert L.sphx_sample_merge(4, C.byref(part), 1, C.byref(wants_fraction)) == bad
    assert b"lacks" in L.sphx_multi_last_error(None)
    assert L.sphx_sample_merge(4, C.byref(part), 1, C.byref(o)) == 0
    with pytest.raises(ValueError):
        ya.sample_merge([])
    with pytest.raises(ValueError):
        ya.sample_merge([dict(density=np.zeros(3, F))])
