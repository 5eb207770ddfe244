"""Fluid statistics of a tiled run (sphx_multi_fluid_stats, sphx_multi_stats_*, sphx_tile_fluid_stats; include/sphx.h), the parts that
need no GPU: the exports, the bindings and the NULL refusals, and the host side of the combination — the fold of the tiles' records and
the encoding that carries them across ranks (yasph2d_amd/csrc/sphx_stats_merge.hpp) — as a stand-alone program built with the address
and undefined-behaviour sanitizers."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import yasph2d_amd as y
from yasph2d_amd import _lib
from yasph2d_amd.multi import MultiSolver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "yasph2d_amd", "csrc")
MULTI_CALLS = ("sphx_multi_fluid_stats", "sphx_multi_stats_record", "sphx_multi_stats_get_status", "sphx_multi_stats_read")
TILE_CALLS = ("sphx_tile_fluid_stats", "sphx_tile_stats_record", "sphx_tile_stats_frame", "sphx_tile_stats_read")


def test_symbols_exported_and_declared(sphx_lib):
    full = open(os.path.join(ROOT, "include", "sphx.h")).read()
    src = re.sub(r"/\*.*?\*/", "", full, flags=re.S)
    for name in MULTI_CALLS + TILE_CALLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, src), f"{name} is not declared in include/sphx.h"
        assert hasattr(sphx_lib, name), f"{name} is not exported by libsphx.so"
        assert name in _lib.SIGNATURES, name
    assert hasattr(sphx_lib, "sphx_solver_multi") and "sphx_solver_multi" in _lib.SIGNATURES
    assert "SPHX_ABI_VERSION 5" in src and sphx_lib.sphx_abi_version() == 5  # additions only
    # the statistics section no longer says that a tiled run has no counterpart, and the contract of the fold is stated
    stats_section = full.split("---- fluid statistics:")[1].split("#define SPHX_STATS_MAX_RECTS")[0]
    assert "no counterpart" not in stats_section and "sphx_multi_fluid_stats" in stats_section
    tiled = full.split("---- fluid statistics of a tiled run")[1].split("int sphx_tile_fluid_stats")[0]
    for needle in ("ASCENDING TILE RANK", "n * 2^-52 * sum|t|", "identical bytes", "ACROSS tilings is not", "COLLECTIVE", "SPHX_ERR_NOT_READY"):
        assert needle in tiled, needle
    for method in ("stats", "stats_record", "stats_status", "stats_frames"):
        assert hasattr(MultiSolver, method) and hasattr(y.DFSPHMultiSolver, method), method
    assert hasattr(y.SphxContext, "tile_stats")


def test_null_arguments_are_refused(sphx_lib):
    L, bad = sphx_lib, _lib.ERR_INVALID_ARGUMENT
    rec = np.zeros(9, y.STATS_DTYPE)
    info = np.zeros(1, y.STATS_FRAME_DTYPE)
    st = _lib.SphxStatsStatus()
    one = (_lib.SphxRect * 1)(_lib.SphxRect(0, 0, 1, 1))
    p, q = rec.ctypes.data, info.ctypes.data
    assert L.sphx_multi_fluid_stats(None, None, 0, 0, p, None) == bad and L.sphx_multi_fluid_stats(None, one, 1, 0, p, p) == bad
    assert L.sphx_multi_stats_record(None, None, 0, 4, 1) == bad and L.sphx_multi_stats_record(None, None, 0, 0, 0) == bad
    assert L.sphx_multi_stats_get_status(None, C.byref(st)) == bad and L.sphx_multi_stats_get_status(None, None) == bad
    assert L.sphx_multi_stats_read(None, 0, 1, p, q) == bad and L.sphx_multi_stats_read(None, 0, 0, None, None) == bad
    assert L.sphx_tile_fluid_stats(None, None, 0, 0, p) == bad and L.sphx_tile_stats_record(None, None, 0, 4, 1) == bad
    assert L.sphx_tile_stats_frame(None, 0.001, 0) == bad and L.sphx_tile_stats_read(None, 0, 1, p, q) == bad
    assert not L.sphx_solver_multi(None)
    assert not rec.tobytes().strip(b"\0") and not info.tobytes().strip(b"\0")  # nothing was written


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to compile the statistics-merge driver"
    exe = str(tmp_path_factory.mktemp("stats_merge") / "stats_merge_driver")
    # (no -ffast-math, no -ffp-contract=fast: the fold's additions are the IEEE ones)
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(ROOT, "tests", "stats_merge_driver.cpp"), "-o", exe])

    def run(*args):
        r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
        return r.returncode, r.stdout, r.stderr

    return run


@pytest.mark.parametrize("check", ["split", "empty", "zeros", "order", "transport"])
def test_stats_merge_host(driver, check):
    """split: the fold of the records of a known set dealt to 1 .. 64 tiles (some empty) has the set's counts and extremes exactly and
    its sums within n * 2^-52 * sum|t|.  empty: a tile that owns nothing is the neutral element (+INF / -INF extremes, zero sums);
    density_valid is the AND.  zeros: -0 wins a minimum, +0 a maximum, in either order.  order: the fold adds in ascending rank — a case
    where the order changes the last bit.  transport: the integer encoding brings back every 64-bit pattern tried (-0.0, +-inf, NaNs,
    0xFFFFFFFFFFFFFFFF) and every encoded value survives a sum with zeros.  The sanitizers stay clean (any report aborts)."""
    rc, out, err = driver(check)
    assert rc == 0 and out.startswith("ok ") and err == "", (out[-2000:], err[-2000:])
    assert int(out.split()[1]) > 0


def test_merge_header_has_no_hip_and_the_library_uses_it():
    src = open(os.path.join(CSRC, "sphx_stats_merge.hpp")).read()
    assert "hip" not in "".join(re.findall(r"#include\s*[<\"]([^>\"]+)", src)).lower()
    tiles = open(os.path.join(CSRC, "sphx_tiles.cpp")).read()
    assert '#include "sphx_stats_merge.hpp"' in tiles and "sphx_stats_host::fold" in tiles and "sphx_stats_host::encode" in tiles
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "-fno-fast-math" in mk and "-ffp-contract=off" in mk and re.search(r"sphx_tiles\.o:.*sphx_stats_merge\.hpp", mk)
