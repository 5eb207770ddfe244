"""The free surface of a tiled run (sphx_multi_surface_contour, include/sphx.h), the parts that need no GPU: the stable merge of the
tiles' segment lists and the apron assembly as a sanitized stand-alone program, the exported sphx_contour_merge through the bindings
against a plain stable sort, its capacity rule, and the exports / bindings / NULL handling."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import yasph2d_amd as ya
from yasph2d_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "yasph2d_amd", "csrc")
F = np.float32
MULTI_CALLS = ("sphx_multi_surface_contour", "sphx_contour_merge")
TILE_CALLS = ("sphx_tile_contour_sample", "sphx_tile_contour_border_fetch", "sphx_tile_contour_cut", "sphx_tile_contour_fetch")


# ------------------------------------------------------------------------------------------------------ 1. the header, sanitized
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to compile the contour-merge driver"
    exe = str(tmp_path_factory.mktemp("contour_merge") / "contour_merge_driver")
    # -ffp-contract=off: the windows come from the unfused x0 + ix * dx (the library is built with the same flag)
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(ROOT, "tests", "contour_merge_driver.cpp"), "-o", exe])

    def run(*args):
        r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
        return r.returncode, r.stdout, r.stderr

    return run


@pytest.mark.parametrize("check,least", [("merge", 400), ("apron", 60)])
def test_contour_merge_host(driver, check, least):
    """merge: seeded parts with disjoint cell sets — saddle cells (two entries with one cell word, whose order is kept), an empty part,
    n_parts == 0 — against a stable sort of their concatenation, at capacities at, above and below the total with sentinels behind the
    capacity.  apron: windows of 2 strips in x, 3 strips in y (a thin one in the middle), a 2 x 2 grid with its own y cuts per column
    and 3 strips in x with a thin middle, over fine (spacing < h), coarse (spacing > 3 h: a tile owns no node), one-node-wide and
    one-node-high lattices: every apron node is found in exactly one other tile's border and carries that node's word, the tiles cut
    every cell once, and a lattice whose node falls in no window (or in two) is reported.  The sanitizers stay clean."""
    rc, out, err = driver(check)
    assert rc == 0 and out.startswith("ok ") and err == "", (out[-2000:], err[-2000:])
    assert int(out.split()[1]) >= least


def test_merge_header_has_no_hip():
    src = open(os.path.join(CSRC, "sphx_contour_merge.hpp")).read()
    assert "hip" not in "".join(re.findall(r"#include\s*[<\"]([^>\"]+)", src)).lower()


# ------------------------------------------------------------------------------------------------------ 2. the exported merge
def random_parts(rng, n_parts, n_cells, empty=None):
    """Ascending cell words dealt to the parts; about one in five is a saddle cell with two segments."""
    words = np.cumsum(rng.integers(1, 9, n_cells)).astype(np.uint32)
    owner = rng.integers(0, max(n_parts, 1), n_cells)
    if empty is not None and n_parts > 1:
        owner[owner == empty] = (empty + 1) % n_parts
    twice = rng.random(n_cells) < 0.2
    parts = []
    for p in range(n_parts):
        mine = owner == p
        cell = np.repeat(words[mine], np.where(twice[mine], 2, 1))
        seg = rng.integers(0, 2**32, (len(cell), 2, 2), dtype=np.uint64).astype(np.uint32).view(F)
        parts.append(dict(segments=seg, cell=cell, tile=np.full(len(cell), p, np.int32), count=len(cell)))
    return parts


def sort_reference(parts):
    cell = np.concatenate([p["cell"] for p in parts]) if parts else np.zeros(0, np.uint32)
    seg = np.concatenate([p["segments"] for p in parts]) if parts else np.zeros((0, 2, 2), F)
    tile = np.concatenate([p["tile"] for p in parts]) if parts else np.zeros(0, np.int32)
    order = np.argsort(cell, kind="stable")
    return seg[order], cell[order], tile[order]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_exported_merge_against_a_stable_sort(sphx_lib):
    rng = np.random.default_rng(31)
    saddles = 0
    for n_parts, n_cells, empty in ((0, 0, None), (1, 50, None), (2, 300, None), (3, 500, 1), (5, 1000, 0), (4, 3, None)):
        parts = random_parts(rng, n_parts, n_cells, empty)
        seg, cell, tile = sort_reference(parts)
        got = ya.contour_merge(parts)
        assert got["count"] == len(cell) == len(got["cell"])
        assert np.array_equal(got["cell"], cell) and np.array_equal(bits(got["segments"]), bits(seg))
        if n_parts:
            assert np.array_equal(got["tile"], tile)
        if empty is not None:
            assert len(parts[empty]["cell"]) == 0
        saddles += int((cell[1:] == cell[:-1]).sum())
        # without tile arrays the result has none; a smaller cap returns the first entries of the same order
        if n_parts:
            sub = ya.contour_merge([{k: v for k, v in p.items() if k != "tile"} for p in parts], cap=len(cell) // 2)
            assert "tile" not in sub and sub["count"] == len(cell) and np.array_equal(sub["cell"], cell[:len(cell) // 2])
            assert np.array_equal(bits(sub["segments"]), bits(seg[:len(cell) // 2]))
    assert saddles > 100


def _struct(seg, cell, tile, count):
    o = _lib.SphxMultiContourOut()
    o.segments, o.cell, o.tile, o.count = (a.ctypes.data if a is not None else None for a in (seg, cell, tile, count))
    o.keep = (seg, cell, tile, count)  # (the struct holds addresses only)
    return o


def test_exported_merge_capacity_rule(sphx_lib):
    """Truncation at cap_segments with a sentinel behind the capacity; a truncated part gives SPHX_ERR_CAPACITY with the count set and
    no segment written.  (out aliases no part: the merge writes entry k before it has read every part's later entries.)"""
    L = sphx_lib
    rng = np.random.default_rng(32)
    parts = random_parts(rng, 3, 400)
    seg, cell, tile = sort_reference(parts)
    total = len(cell)
    counts = [np.array([p["count"]], np.uint32) for p in parts]
    arr = (_lib.SphxMultiContourOut * 3)(*[_struct(p["segments"], p["cell"], p["tile"], c) for p, c in zip(parts, counts)])
    stored = np.array([p["count"] for p in parts], np.uint32)
    sp = stored.ctypes.data_as(C.POINTER(C.c_uint32))
    for cap in (0, 1, total - 1, total, total + 7):
        room = cap + 4
        o_seg, o_cell, o_tile, o_cnt = np.full((room, 4), -7.0, F), np.full(room, 0xDEADBEEF, np.uint32), np.full(room, -77, np.int32), np.zeros(1, np.uint32)
        assert L.sphx_contour_merge(arr, sp, 3, cap, C.byref(_struct(o_seg, o_cell, o_tile, o_cnt))) == 0
        n = min(cap, total)
        assert o_cnt[0] == total
        assert np.array_equal(o_cell[:n], cell[:n]) and np.array_equal(o_tile[:n], tile[:n]) and np.array_equal(bits(o_seg[:n]), bits(seg[:n]).reshape(n, 4))
        assert (o_cell[n:] == 0xDEADBEEF).all() and (o_tile[n:] == -77).all() and (o_seg[n:] == -7.0).all()
    # part 1 holds fewer entries than its count
    short = stored.copy()
    short[1] -= 1
    o_seg, o_cell, o_tile, o_cnt = np.full((total, 4), -7.0, F), np.full(total, 0xDEADBEEF, np.uint32), np.full(total, -77, np.int32), np.zeros(1, np.uint32)
    rc = L.sphx_contour_merge(arr, short.ctypes.data_as(C.POINTER(C.c_uint32)), 3, total, C.byref(_struct(o_seg, o_cell, o_tile, o_cnt)))
    assert rc == _lib.ERR_CAPACITY and o_cnt[0] == total
    assert (o_cell == 0xDEADBEEF).all() and (o_tile == -77).all() and (o_seg == -7.0).all()
    with pytest.raises(ya.SphxError) as e:
        ya.contour_merge([dict(p, segments=p["segments"][:-1], cell=p["cell"][:-1], tile=p["tile"][:-1]) if k == 1 else p for k, p in enumerate(parts)])
    assert e.value.code == _lib.ERR_CAPACITY and e.value.count == total
    # no part at all: count 0, nothing written
    o_cnt[0] = 99
    assert L.sphx_contour_merge(None, None, 0, total, C.byref(_struct(o_seg, o_cell, o_tile, o_cnt))) == 0
    assert o_cnt[0] == 0 and (o_cell == 0xDEADBEEF).all()
    assert ya.contour_merge([])["count"] == 0


def test_merged_segments_chain_like_the_whole(sphx_lib):
    """contour_lines takes the merged segments as they are: a closed square cut into two parts chains to one closed line."""
    pts = np.array([[0, 0], [1, 0], [1, 1], [0, 1]], F)
    seg = np.stack([pts, np.roll(pts, -1, 0)], 1)  # four segments round the square
    cell = np.array([3, 9, 12, 20], np.uint32)
    parts = [dict(segments=seg[[0, 2]], cell=cell[[0, 2]], count=2), dict(segments=seg[[1, 3]], cell=cell[[1, 3]], count=2)]
    got = ya.contour_merge(parts)
    assert np.array_equal(got["cell"], cell) and np.array_equal(got["segments"], seg)
    lines, closed = ya.contour_lines(got["segments"])
    assert len(lines) == 1 and closed[0]


# ------------------------------------------------------------------------------------------------------ 3. exports, bindings, NULL
def test_header_declares_and_library_exports(sphx_lib):
    full = open(os.path.join(ROOT, "include", "sphx.h")).read()
    src = re.sub(r"/\*.*?\*/", "", full, flags=re.S)
    for name in MULTI_CALLS + TILE_CALLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, src), f"{name} is not declared in include/sphx.h"
        assert hasattr(sphx_lib, name), f"{name} is not exported by libsphx.so"
        assert name in _lib.SIGNATURES
    assert sphx_lib.sphx_abi_version() == 5
    assert "SPHX_ABI_VERSION 5" in src and re.search(r"5 \(additive\): sphx_multi_surface_contour", full)
    assert "free surface of a tiled run" in full
    assert C.sizeof(_lib.SphxMultiContourOut) == 4 * C.sizeof(C.c_void_p)
    from yasph2d_amd.multi import MultiSolver

    assert callable(MultiSolver.contour) and callable(ya.DFSPHMultiSolver.contour) and "contour_merge" in ya.__all__
    assert "does not exist yet" not in open(os.path.join(ROOT, "README.md")).read()


def test_null_and_bad_arguments_are_refused(sphx_lib):
    L, bad = sphx_lib, _lib.ERR_INVALID_ARGUMENT
    cnt = np.zeros(1, np.uint32)
    cel = np.zeros(4, np.uint32)
    o = _struct(None, cel, None, cnt)
    win = (C.c_uint32 * 4)()
    assert L.sphx_multi_surface_contour(None, 0.0, 0.0, 0.1, 0.1, 4, 4, 0, 0, 0.5, 4, 0, C.byref(o)) == bad
    assert L.sphx_tile_contour_sample(None, 0.0, 0.0, 0.1, 0.1, 4, 4, 0, 0, win) == bad
    assert L.sphx_tile_contour_border_fetch(None, None, 0) == bad
    assert L.sphx_tile_contour_cut(None, 0.5, 4, None, 0) == bad
    assert L.sphx_tile_contour_fetch(None, None, None, C.byref(C.c_uint32())) == bad
    # the merge: out NULL, out->count NULL, parts NULL with n_parts > 0, a part without count or cell, stored above the count
    one = np.array([1], np.uint32)
    sp = one.ctypes.data_as(C.POINTER(C.c_uint32))
    part = _struct(np.zeros((1, 4), F), cel, None, np.array([1], np.uint32))
    assert L.sphx_contour_merge(C.byref(part), sp, 1, 4, None) == bad
    assert b"out is NULL" in L.sphx_multi_last_error(None)
    assert L.sphx_contour_merge(C.byref(part), sp, 1, 4, C.byref(_struct(None, cel, None, None))) == bad
    assert L.sphx_contour_merge(None, sp, 1, 4, C.byref(o)) == bad
    assert L.sphx_contour_merge(C.byref(part), None, 1, 4, C.byref(o)) == bad
    assert L.sphx_contour_merge(C.byref(_struct(None, cel, None, None)), sp, 1, 4, C.byref(o)) == bad
    assert L.sphx_contour_merge(C.byref(_struct(None, None, None, np.array([1], np.uint32))), sp, 1, 4, C.byref(o)) == bad
    assert b"cell" in L.sphx_multi_last_error(None)
    assert L.sphx_contour_merge(C.byref(_struct(None, cel, None, np.array([0], np.uint32))), sp, 1, 4, C.byref(o)) == bad
    wants_seg = _struct(np.zeros((4, 4), F), cel, None, cnt)
    assert L.sphx_contour_merge(C.byref(_struct(None, cel, None, np.array([1], np.uint32))), sp, 1, 4, C.byref(wants_seg)) == bad
    assert b"lacks" in L.sphx_multi_last_error(None)
    assert L.sphx_contour_merge(C.byref(part), sp, 1, 4, C.byref(o)) == 0 and cnt[0] == 1
