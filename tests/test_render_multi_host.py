"""The picture of a tiled run (sphx_multi_render, sphx_multi_render_layer, sphx_render_merge, sphx_tile_render_layer; include/sphx.h),
the parts that need no GPU: the exports and bindings, sphx_render_merge against the numpy restatement of the composite rule
(tests/render_multi_reference.py), the merge and window headers as a stand-alone program under the address and undefined-behaviour
sanitizers (tests/render_merge_driver.cpp), and the rule itself: on the golden states, cut into tiles, the composite of the tiles'
layers is the single context's picture — with views that put the seams under load."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import render_multi_reference as rm
import render_reference as rr
import yasph2d_amd as y
from tiles_reference import GridLayout, StripLayout, cell_coord, quantile_cuts
from yasph2d_amd import _lib
from yasph2d_amd.multi import MultiSolver

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "yasph2d_amd", "csrc")
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "dam_break_4050.npz"))
CALLS = ("sphx_multi_render", "sphx_multi_render_layer", "sphx_render_merge", "sphx_tile_render_layer", "sphx_tile_render_window")
NONE, BOUNDARY = rm.NONE, rm.BOUNDARY


def test_symbols_exported_and_declared(sphx_lib):
    full = open(os.path.join(ROOT, "include", "sphx.h")).read()
    src = re.sub(r"/\*.*?\*/", "", full, flags=re.S)
    for name in CALLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, src), f"{name} is not declared in include/sphx.h"
        assert hasattr(sphx_lib, name), f"{name} is not exported by libsphx.so"
        assert name in _lib.SIGNATURES, name
    assert "SPHX_ABI_VERSION 5" in src and sphx_lib.sphx_abi_version() == 5  # additions only
    assert C.sizeof(_lib.SphxRenderLayer) == 24
    section = full.split("---- picture of a tiled run")[1].split("typedef struct sphx_render_layer")[0]
    for needle in ("COMPOSITE RULE", "STRICTLY greater", "particle ID", "sphx_render_merge", "rank mode", "SPHX_ERR_NOT_READY", "No side effects", "window"):
        assert needle in section, needle
    for method in ("render", "render_layer"):
        assert hasattr(MultiSolver, method) and hasattr(y.DFSPHMultiSolver, method), method
    assert callable(y.render_merge)
    # NULL handles are refused before anything is read
    v = y.render_fit(8, 8)
    bad = _lib.ERR_INVALID_ARGUMENT
    assert sphx_lib.sphx_multi_render(None, C.byref(v), 0, None) == bad and sphx_lib.sphx_multi_render_layer(None, C.byref(v), 0, None) == bad
    assert sphx_lib.sphx_tile_render_layer(None, C.byref(v), 0, None) == bad and sphx_lib.sphx_tile_render_window(None, C.byref(v), 1, None, None) == bad


def test_headers_have_no_hip_and_the_library_uses_them():
    for name in ("sphx_render_merge.hpp", "sphx_render_window.hpp"):
        src = open(os.path.join(CSRC, name)).read()
        assert "hip" not in "".join(re.findall(r"#include\s*[<\"]([^>\"]+)", src)).lower()
    tiles = open(os.path.join(CSRC, "sphx_tiles.cpp")).read()
    assert "sphx_render_merge.hpp" in tiles and "fold_window" in tiles and "sphx_render_host::merge(" in tiles
    render = open(os.path.join(CSRC, "sphx_render.inc")).read()
    assert "sphx_render_window.hpp" in render and "render_tile_window(" in render and render.count("render_view_error(") >= 2


# ---- sphx_render_merge through ctypes ------------------------------------------------------------------------------------------------------
def c_layer(l):
    return _lib.SphxRenderLayer(l["key"].ctypes.data, l["owner"].ctypes.data, l["rgba"].ctypes.data if l.get("rgba") is not None else None)


def c_merge(L, layers, w, h, rgba=True, out=None):
    arr = (_lib.SphxRenderLayer * max(len(layers), 1))(*[c_layer(l) for l in layers])
    if out is None:
        out = dict(key=np.full((h, w), 77, np.uint32), owner=np.full((h, w), 77, np.uint32))
        if rgba:
            out["rgba"] = np.full((h, w, 4), 77, np.uint8)
    rc = L.sphx_render_merge(w, h, arr, len(layers), C.byref(c_layer(out)))
    return rc, out


def same(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in b)


def hand_layer(owner, key, colour):
    o = np.array(owner, np.uint32).reshape(2, -1)
    rgba = np.zeros(o.shape + (4,), np.uint8)
    rgba[:] = colour
    return dict(key=np.array(key, np.uint32).reshape(o.shape), owner=o, rgba=rgba)


def test_merge_hand_made_layers(sphx_lib):
    """fluid over boundary over none in both layer orders; of two fluid owners the greater key whichever comes first; equal keys keep the
    earlier layer; rgba follows the owner"""
    a = hand_layer([7, BOUNDARY, NONE, 7, 5, NONE], [5, 0, 0, 5, 9, 0], 0xA0)
    b = hand_layer([BOUNDARY, NONE, 9, 8, 6, NONE], [0, 0, 1, 5, 3, 0], 0xB0)
    for order, (l0, l1) in enumerate(((a, b), (b, a))):
        rc, got = c_merge(sphx_lib, [l0, l1], 3, 2)
        assert rc == _lib.OK and same(got, rm.merge([l0, l1]))
        assert got["owner"].ravel().tolist() == [7, BOUNDARY, 9, 8 if order else 7, 5, NONE]
        assert got["key"].ravel().tolist() == [5, 0, 1, 5, 9, 0]
        first, second = (0xB0, 0xA0) if order else (0xA0, 0xB0)
        assert got["rgba"][..., 0].ravel().tolist() == [0xA0, 0xA0, 0xB0, first, 0xA0, first]  # (none over none: the earlier layer's background)
        assert (got["rgba"] == got["rgba"][..., :1]).all()  # no pixel mixes the bytes of two layers
        assert second in (0xA0, 0xB0)


@pytest.mark.parametrize("shape", [(1, 1), (7, 1), (1, 5), (23, 37), (16, 16)])
def test_merge_random_layers_aliasing_and_layer_counts(sphx_lib, shape):
    h, w = shape
    rng = np.random.default_rng(h * 100 + w)

    def layer(tag):
        kind = rng.integers(0, 4, (h, w))
        owner = np.where(kind == 0, NONE, np.where(kind == 1, BOUNDARY, rng.integers(0, 1000, (h, w)))).astype(np.uint32)
        key = np.where(kind >= 2, rng.integers(0, 6, (h, w)), 0).astype(np.uint32)  # few values: equal keys are common
        rgba = (tag * 16 + rng.integers(0, 16, (h, w, 4))).astype(np.uint8)
        return dict(key=key, owner=owner, rgba=rgba)

    for n in (1, 2, 3, 5, 8):
        layers = [layer(t) for t in range(n)]
        want = rm.merge(layers)
        rc, got = c_merge(sphx_lib, layers, w, h)
        assert rc == _lib.OK and same(got, want), n
        if n == 1:
            assert same(got, layers[0])
        # without colours, and key / owner alone
        rc, got = c_merge(sphx_lib, [dict(key=l["key"], owner=l["owner"]) for l in layers], w, h, rgba=False)
        assert rc == _lib.OK and same(got, dict(key=want["key"], owner=want["owner"]))
        # out aliases layers[0]
        first = {k: v.copy() for k, v in layers[0].items()}
        rc, got = c_merge(sphx_lib, [first] + layers[1:], w, h, out=first)
        assert rc == _lib.OK and same(first, want)
        # the Python wrapper
        assert same(y.render_merge(layers), want)
    # no layer: the picture shows nothing
    rc, got = c_merge(sphx_lib, [], w, h, rgba=False)
    assert rc == _lib.OK and (got["owner"] == NONE).all() and (got["key"] == 0).all()


def test_merge_argument_errors(sphx_lib):
    L, bad = sphx_lib, _lib.ERR_INVALID_ARGUMENT
    a = hand_layer([1, 2, 3, 4], [1, 2, 3, 4], 9)
    out = hand_layer([0] * 4, [0] * 4, 0)
    before = {k: v.copy() for k, v in out.items()}
    one = (_lib.SphxRenderLayer * 1)(c_layer(a))

    def err(rc, needle):
        msg = L.sphx_multi_last_error(None).decode()
        assert rc == bad and "sphx_render_merge" in msg and needle in msg, (rc, msg)

    err(L.sphx_render_merge(2, 2, one, 1, None), "out is NULL")
    err(L.sphx_render_merge(2, 2, one, 1, C.byref(_lib.SphxRenderLayer(None, None, None))), "no output")
    err(L.sphx_render_merge(2, 2, None, 1, C.byref(c_layer(out))), "layers is NULL")
    for k in ("key", "owner"):
        broken = c_layer(a)
        setattr(broken, k, None)
        err(L.sphx_render_merge(2, 2, (_lib.SphxRenderLayer * 1)(broken), 1, C.byref(c_layer(out))), "key or owner")
    err(L.sphx_render_merge(2, 2, (_lib.SphxRenderLayer * 1)(c_layer(dict(key=a["key"], owner=a["owner"]))), 1, C.byref(c_layer(out))), "rgba")
    err(L.sphx_render_merge(1 << 14, 1 << 14, one, 1, C.byref(c_layer(out))), "2^28")
    err(L.sphx_render_merge(0xFFFFFFFF, 0xFFFFFFFF, one, 1, C.byref(c_layer(out))), "2^28")
    err(L.sphx_render_merge(2, 2, None, 0, C.byref(c_layer(out))), "background")
    assert same(out, before)  # a refused call writes nothing
    assert L.sphx_render_merge(0, 0, None, 0, C.byref(c_layer(dict(key=out["key"], owner=out["owner"])))) == _lib.OK and same(out, before)
    with pytest.raises(ValueError):
        y.render_merge([])
    with pytest.raises(ValueError):
        y.render_merge([a, hand_layer([1, 2], [1, 2], 0)])


# ---- the headers under the sanitizers ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to compile the render-merge driver"
    exe = str(tmp_path_factory.mktemp("render_merge") / "render_merge_driver")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(ROOT, "tests", "render_merge_driver.cpp"), "-o", exe])

    def run(*args):
        r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
        return r.returncode, r.stdout, r.stderr

    return run


@pytest.mark.parametrize("check", ["merge", "window"])
def test_merge_and_window_headers_under_sanitizers(driver, check):
    """merge: the fold against a pairwise restatement (1 x 1 and odd sizes, equal keys, aliasing, 0 / 1 layers, argument errors) and
    fold_window against the fold of the padded window.  window: whatever the camera, the grid and the rectangle (+-1e30, NaN, +-inf,
    rectangles touching 0 and 65536, 1 x 1 and odd images) a window stays inside its image, and no pixel a particle covers lies outside
    the window of a rectangle that holds the particle's cell."""
    rc, out, err = driver(check)
    print(out)
    assert rc == 0 and "ok " + check in out and "FAILED" not in out, out[-3000:] + err[-3000:]


# ---- the rule on the golden states -------------------------------------------------------------------------------------------------------------
def golden_state(step):
    # (a single context issues ids in upload order; any injective labelling serves the comparison)
    return dict(pos=GOLD["s%d_pos" % step], vel=GOLD["s%d_vel" % step], boundary=GOLD["in_boundary"], ids=GOLD["s%d_ids" % step])


def tilings(pos):
    cx = cell_coord(pos, 0)
    return {"2 strips": StripLayout(0, quantile_cuts(cx, 2)).rects(), "3 strips": StripLayout(0, quantile_cuts(cx, 3)).rects(),
            "2 x 2": GridLayout.quantile(pos, 2, 2).rects()}


def seam_view(rects, pos):
    """a zoom onto the first cut at radius = smoothing_length: the world point where the first two rectangles meet along x, at the
    fluid's median height, 2000 pixels per unit"""
    x = -100.0 + rects[0][1] * 0.02
    return rr.View(160, 120, (x, float(np.median(pos[:, 1]))), 2000.0, radius=rm.SMOOTHING_LENGTH)


@pytest.mark.parametrize("step", [10, 100])
def test_the_composite_of_the_tiles_is_the_single_picture(step):
    st = golden_state(step)
    keys = rm.cell_keys(st["pos"]).astype(np.int64)
    assert (np.diff(keys) >= 0).all(), "the golden device order is not ascending in morton(cell_of(pos))"
    ids = np.asarray(st["ids"], np.uint32)
    assert len(np.unique(ids)) == len(ids) and (ids < (1 << 31)).all()
    whole = {}
    for name, rects in tilings(st["pos"]).items():
        tiles = rm.split(st, rects)
        assert sum(len(t["ids"]) for t, _ in tiles) == len(ids) and sum(len(b) for _, b in tiles) == len(st["boundary"])
        assert all(len(t["ids"]) > 0 for t, _ in tiles)
        views = {"radius 0.015": rr.fit(320, 240, radius=0.015), "reference radius": rr.fit(320, 240), "seam zoom": seam_view(rects, st["pos"])}
        for vname, view in views.items():
            vkey = vname if vname != "seam zoom" else (vname, rects[0][1])
            if vkey not in whole:
                w = rr.render32(st, view, rm.PARTICLE_RADIUS)
                fluid = w["owner"] < BOUNDARY
                w["ids"] = np.where(fluid, ids[np.where(fluid, w["owner"], 0)], w["owner"]).astype(np.uint32)
                whole[vkey] = w
            want = whole[vkey]
            layers = [rm.layer32(t, b, view, rect=r) for (t, b), r in zip(tiles, rects)]
            got = rm.merge(layers)
            what = "s%d, %s, %s" % (step, name, vname)
            assert np.array_equal(got["owner"], want["ids"]), what
            assert np.array_equal(got["rgba"], want["rgba"]), what
            fl = got["owner"] < BOUNDARY
            assert (got["key"][~fl] == 0).all() and fl.any(), what
            if vname != "seam zoom":  # (the zoom is inside the fluid)
                assert (got["owner"] == BOUNDARY).any() and (got["owner"] == NONE).any(), what
            # no two competing layers carry the same key
            k = np.stack([np.where(l["owner"] < BOUNDARY, l["key"].astype(np.int64), -1 - i) for i, l in enumerate(layers)])
            k.sort(axis=0)
            assert ((k[1:] != k[:-1]) | (k[1:] < 0)).all(), what
            multi, not_lowest, not_highest = rm.seam_counts(layers)
            print("%s: %d pixels covered by two or more tiles, winner not the lowest rank at %d, not the highest at %d" % (what, multi, not_lowest, not_highest))
            if vname == "radius 0.015":  # the scene's power (conditions, not tolerances): either naive merge order would fail
                assert multi >= 100 and not_lowest >= 20 and not_highest >= 20, what
