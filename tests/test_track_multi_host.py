"""Following particles by id in a tiled run (sphx_multi_track_*, sphx_multi_download_by_id, include/sphx.h), the parts that need no
GPU: the host merge as a sanitized stand-alone program, the exported merge through the bindings against a numpy restatement, and the
exports / bindings / NULL handling of the new calls."""
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
MULTI_CALLS = ("sphx_multi_track_set", "sphx_multi_track_fetch", "sphx_multi_track_record", "sphx_multi_track_get_status", "sphx_multi_track_read",
               "sphx_multi_download_by_id", "sphx_track_merge", "sphx_track_merge_frames")
TILE_CALLS = ("sphx_tile_track_install", "sphx_tile_track_fetch_enqueue", "sphx_tile_track_fetch", "sphx_tile_track_window_enqueue",
              "sphx_tile_track_window_fetch", "sphx_tile_track_record", "sphx_tile_track_frame", "sphx_tile_track_read")
A, W = 0xFFFFFFFF, 0x7FC00000


# ------------------------------------------------------------------------------------------------------ 1. the merge header, sanitized
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to compile the track-merge driver"
    exe = str(tmp_path_factory.mktemp("track_merge") / "track_merge_driver")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, os.path.join(ROOT, "tests", "track_merge_driver.cpp"), "-o", exe])

    def run(*args):
        r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
        return r.returncode, r.stdout, r.stderr

    return run


@pytest.mark.parametrize("check", ["random", "empty", "absent", "two", "scatter", "capacity", "nanbits", "frames", "checks"])
def test_track_merge_host(driver, check):
    """random: the merge against a brute-force restatement on random parts.  empty: no parts, zero entries, a tile without records.
    absent: all-absent parts.  two: an id held by two parts (the greatest (tile, slot) wins, an equal pair keeps the earlier part).
    scatter: packed window records in shuffled order, subsets of the outputs, a record outside the window.  capacity: as many records
    as the buffer holds.  nanbits: a particle whose floats are all 0x7FC00000 stays present.  frames: the fold of frames.  checks: the
    argument checks.  The sanitizers stay clean (any report aborts the program)."""
    rc, out, err = driver(check)
    assert rc == 0 and out.startswith("ok ") and err == "", (out[-2000:], err[-2000:])
    assert int(out.split()[1]) > 0


def test_track_merge_header_has_no_hip():
    src = open(os.path.join(CSRC, "sphx_track_merge.hpp")).read()
    assert "hip" not in "".join(re.findall(r"#include\s*[<\"]([^>\"]+)", src)).lower()


# ------------------------------------------------------------------------------------------------------ 2. the exported merge
def words(a):
    return a.view(np.uint32)  # (float32 or uint32 arrays: the bits)


def random_part(rng, m, tile, p_present):
    part = dict(tile=np.full(m, A, np.uint32), slot=np.full(m, A, np.uint32), pos=np.full((m, 2), W, np.uint32).view(np.float32),
                vel=np.full((m, 2), W, np.uint32).view(np.float32), density=np.full(m, W, np.uint32).view(np.float32))
    on = rng.random(m) < p_present
    part["tile"][on] = tile
    part["slot"][on] = rng.integers(0, 50, on.sum())
    for f in ("pos", "vel", "density"):
        words(part[f])[on] = rng.integers(0, 2**32, (on.sum(),) + part[f].shape[1:], dtype=np.uint64).astype(np.uint32)
    return part


def merge_reference(parts):
    m = len(parts[0]["tile"])
    out = random_part(np.random.default_rng(0), m, 0, 0.0)
    key = np.full(m, -1, np.int64)
    for p in parts:
        k = np.where(p["tile"] == A, -1, p["tile"].astype(np.int64) * 2**32 + p["slot"])
        take = k > key
        key[take] = k[take]
        for f in out:
            words(out[f])[take] = words(p[f])[take]
    return out, int((key >= 0).sum())


def test_exported_merge_against_numpy(sphx_lib):
    rng = np.random.default_rng(11)
    for m, n_parts in ((0, 2), (1, 1), (257, 2), (1000, 5)):
        parts = [random_part(rng, m, int(rng.integers(0, 4)), 0.4) for _ in range(n_parts)]
        want, present = merge_reference(parts)
        got = ya.track_merge(parts)
        assert got.pop("present") == present
        for f in want:
            assert np.array_equal(words(got[f]), words(want[f])), f
        # a subset of the fields gives the same bits
        sub = ya.track_merge([{f: p[f] for f in ("tile", "slot", "vel")} for p in parts])
        assert sub["present"] == present and np.array_equal(words(sub["vel"]), words(want["vel"])) and "pos" not in sub
    # a particle whose floats are all the absent word is present
    p = random_part(rng, 3, 1, 0.0)
    p["tile"][1], p["slot"][1] = 1, 4
    assert ya.track_merge([p, random_part(rng, 3, 0, 0.0)])["present"] == 1


def test_exported_merge_frames_against_numpy(sphx_lib):
    rng = np.random.default_rng(12)
    for shape, n_parts in (((0, 5), 2), ((3, 0), 2), ((4, 33), 1), ((5, 200), 4)):
        parts = []
        for k in range(n_parts):
            t = np.where(rng.random(shape) < 0.4, k, A).astype(np.uint32)
            parts.append((rng.integers(0, 2**32, shape + (4,), dtype=np.uint64).astype(np.uint32).view(np.float32), t))
        out, til = ya.track_merge_frames(parts)
        want, want_t = np.full(shape + (4,), W, np.uint32), np.full(shape, A, np.uint32)
        for f, t in parts:  # (ascending tile: a later part always wins where it is present)
            on = t != A
            want[on], want_t[on] = words(f)[on], t[on]
        assert np.array_equal(words(out), want) and np.array_equal(til, want_t)


# ------------------------------------------------------------------------------------------------------ 3. exports, bindings, NULL
def test_header_declares_and_library_exports(sphx_lib):
    full = open(os.path.join(ROOT, "include", "sphx.h")).read()
    src = re.sub(r"/\*.*?\*/", "", full, flags=re.S)
    for name in MULTI_CALLS + TILE_CALLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, src), f"{name} is not declared in include/sphx.h"
        assert hasattr(sphx_lib, name), f"{name} is not exported by libsphx.so"
        assert name in _lib.SIGNATURES
    assert "SPHX_ABI_VERSION 5" in src and re.search(r"5 \(additive\): sphx_multi_track_set", full)
    assert "following particles by id in a tiled run" in full
    assert C.sizeof(_lib.SphxMultiTrackOut) == 5 * C.sizeof(C.c_void_p)


def test_null_and_bad_arguments_are_refused(sphx_lib):
    L, bad = sphx_lib, _lib.ERR_INVALID_ARGUMENT
    ids = (C.c_uint32 * 4)(1, 2, 3, 4)
    buf = (C.c_float * 64)()
    til = (C.c_uint32 * 16)()
    o = _lib.SphxMultiTrackOut(C.addressof(til), None, C.addressof(buf), None, None)
    st = _lib.SphxTrackStatus()
    n = C.c_uint32(123)
    assert L.sphx_multi_track_set(None, ids, 4) == bad and L.sphx_multi_track_set(None, None, 0) == bad
    assert L.sphx_multi_track_fetch(None, 0, C.byref(o)) == bad and L.sphx_multi_track_fetch(None, 0, None) == bad
    assert L.sphx_multi_track_record(None, 10, 1) == bad and L.sphx_multi_track_record(None, 0, 0) == bad
    assert L.sphx_multi_track_get_status(None, C.byref(st)) == bad and L.sphx_multi_track_get_status(None, None) == bad
    assert L.sphx_multi_track_read(None, 0, 1, 0, buf, til) == bad and L.sphx_multi_track_read(None, 0, 0, 0, None, None) == bad
    assert L.sphx_multi_download_by_id(None, 0, 4, 0, C.byref(o), C.byref(n)) == bad and L.sphx_multi_download_by_id(None, 0, 0, 0, None, None) == bad
    for name in TILE_CALLS:  # (a NULL context is refused by every tile call before anything else)
        args = [None] + [0 if t in (C.c_uint32, C.c_float) else None for t in _lib.SIGNATURES[name][1][1:]]
        assert getattr(L, name)(*args) == bad, name
    # the merge: out NULL, every output NULL, a part without tile / slot, an array a part lacks
    part = _lib.SphxMultiTrackOut(C.addressof(til), C.addressof(til), C.addressof(buf), None, None)
    none = _lib.SphxMultiTrackOut()
    assert L.sphx_track_merge(4, C.byref(part), 1, None, None) == bad and b"out is NULL" in L.sphx_multi_last_error(None)
    assert L.sphx_track_merge(4, C.byref(part), 1, C.byref(none), None) == bad
    assert L.sphx_track_merge(4, None, 1, C.byref(o), None) == bad
    assert L.sphx_track_merge(4, C.byref(o), 1, C.byref(o), None) == bad and b"tile or slot" in L.sphx_multi_last_error(None)
    want_vel = _lib.SphxMultiTrackOut(None, None, None, C.addressof(buf), None)
    assert L.sphx_track_merge(4, C.byref(part), 1, C.byref(want_vel), None) == bad and b"lacks" in L.sphx_multi_last_error(None)
    ptrs = (C.c_void_p * 1)(C.addressof(buf))
    tptr = (C.c_void_p * 1)(C.addressof(til))
    assert L.sphx_track_merge_frames(4, ptrs, tptr, 1, None, None) == bad
    assert L.sphx_track_merge_frames(4, None, tptr, 1, buf, None) == bad
    assert L.sphx_track_merge_frames(4, (C.c_void_p * 1)(None), tptr, 1, buf, None) == bad
    assert n.value == 123 and not any(buf) and not any(til)
    # ... and the good case with no parts: everything absent
    assert L.sphx_track_merge(4, None, 0, C.byref(o), C.byref(n)) == 0 and n.value == 0
    assert list(til)[:4] == [A] * 4 and np.frombuffer(buf, np.uint32)[:8].tolist() == [W] * 8


def test_python_surface():
    from yasph2d_amd.multi import MultiSolver

    for cls in (MultiSolver, ya.DFSPHMultiSolver):
        for name in ("track", "track_fetch", "track_record", "track_status", "track_frames", "download_by_id"):
            assert callable(getattr(cls, name)), (cls, name)
    assert callable(ya.track_merge) and callable(ya.track_merge_frames)
    with pytest.raises(ValueError):
        ya.track_merge([])
    with pytest.raises(ValueError):
        ya.track_merge_frames([])
