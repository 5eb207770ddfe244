"""Gauges of a tiled run without a GPU: the two facts the design rests on, held before any kernel runs.

1. The owned samples of one tile on one gauge are one contiguous index interval: the bisection of csrc/sphx_gauge_window.hpp
   (tests/gauge_merge_driver.cpp, compiled alone under the address and undefined-behaviour sanitizers) equals the brute-force owned set of
   tests/gauge_multi_reference.py on the grids of tests/constants_scenes.py, for strips and 2 x 2 rectangles, rays of every direction,
   zero steps, rays that leave the domain and steps that overflow; every sample is owned exactly once.
2. The fold of the tiles' 32-byte parts (csrc/sphx_gauge_merge.hpp: the driver and the library's sphx_gauge_merge) equals the gauge rule
   over the concatenated values bit for bit, at every position of a cut relative to `last`; mutants of the fold are rejected; a gap, an
   overlap and a wrong count are refused."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import constants_scenes as cs
import gauge_multi_reference as gmr
import gauge_reference as gr
import yasph2d_amd as y
from yasph2d_amd import _lib

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "yasph2d_amd", "csrc")
NAN = F(np.nan)
NEW_SYMBOLS = ("sphx_multi_gauge_levels", "sphx_gauge_merge", "sphx_multi_probe_record", "sphx_multi_probe_get_status", "sphx_multi_probe_read",
               "sphx_tile_gauge_levels", "sphx_tile_gauge_fetch", "sphx_tile_probe_record", "sphx_tile_probe_due", "sphx_tile_probe_frame",
               "sphx_tile_probe_read")


def test_multi_gauge_symbols_and_abi(sphx_lib):
    for name in NEW_SYMBOLS:
        assert hasattr(sphx_lib, name) and name in _lib.SIGNATURES, name
    full = open(os.path.join(ROOT, "include", "sphx.h")).read()
    assert re.search(r"#define SPHX_ABI_VERSION 5\b", full) and sphx_lib.sphx_abi_version() == 5  # additions only
    assert re.search(r"5 \(additive\): sphx_multi_gauge_levels, ", full)
    assert y.GAUGE_PART_DTYPE.itemsize == 32 and y.GAUGE_PART_DTYPE == gmr.PART_DTYPE
    from yasph2d_amd.multi import MultiSolver

    for name in ("gauges", "probe_record", "probe_status", "probe_frames"):
        assert callable(getattr(MultiSolver, name)) and callable(getattr(y.DFSPHMultiSolver, name))
    assert callable(y.gauge_merge) and "gauge_merge" in y.__all__
    st = _lib.SphxProbeStatus()
    assert sphx_lib.sphx_multi_gauge_levels(None, None, 0, 0, 0, 0.5, 0, None, None, None) == _lib.ERR_INVALID_ARGUMENT
    assert sphx_lib.sphx_multi_probe_record(None, None, 0, None, 0, 0, 0, 0.5, 4, 1) == _lib.ERR_INVALID_ARGUMENT
    assert sphx_lib.sphx_multi_probe_get_status(None, C.byref(st)) == _lib.ERR_INVALID_ARGUMENT
    assert sphx_lib.sphx_multi_probe_read(None, 0, 0, None, None, None, None) == _lib.ERR_INVALID_ARGUMENT


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "a C++ compiler is needed to compile the gauge-merge driver"
    d = tmp_path_factory.mktemp("gauge_merge")
    exe = str(d / "gauge_merge_driver")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(ROOT, "tests", "gauge_merge_driver.cpp"), "-o", exe])

    def run(mode, payload=None, dtype=None):
        if mode == "self":
            r = subprocess.run([exe, "self"], capture_output=True, text=True, timeout=300)
            assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
            return r.stdout
        src, dst = str(d / "in.bin"), str(d / "out.bin")
        with open(src, "wb") as f:
            f.write(payload)
        r = subprocess.run([exe, mode, src, dst], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
        return r.stdout, np.fromfile(dst, dtype)

    return run


def test_driver_self_test(driver):
    out = driver("self")
    assert out.startswith("ok ") and int(out.split()[1]) > 40000


# ------------------------------------------------------------------------------------------------------------- contiguity
def grid_of(name):
    """-> (grid_min [2], fl(1 / h)) of the app's constants ("app") or of a set of constants_scenes"""
    if name == "app":
        p = y.default_params()
        return np.array(p.grid_min[:], F), F(F(1.0) / F(p.smoothing_length))
    return np.array(cs.SETS[name][4], F), F(F(1.0) / cs.properties(name)["smoothing_length"])


def tilings(gmin, inv):
    """2 strips, 3 strips (along x and along y) and a 2 x 2 layout whose cuts pass through the scene around (0.5, 0.3)"""
    cx, cy = (int(v) for v in gmr.cells(np.array([[0.5, 0.3]], F), gmin, inv)[0])
    W = 65536
    return {
        "2 strips": [(0, cx, 0, W), (cx, W, 0, W)],
        "3 strips": [(0, cx - 7, 0, W), (cx - 7, cx + 9, 0, W), (cx + 9, W, 0, W)],
        "3 strips along y": [(0, W, 0, cy - 2), (0, W, cy - 2, cy + 11), (0, W, cy + 11, W)],
        "2 x 2": [(0, cx, 0, cy), (0, cx, cy, W), (cx, W, 0, cy + 3), (cx, W, cy + 3, W)],
    }


def rays(gmin, inv):
    """vertical, horizontal and oblique rays, negative and zero steps, rays that leave the domain on both sides, steps that overflow"""
    h = float(F(1.0) / inv)
    g = []
    for n in (1, 2, 63, 64, 65, 129, 300):
        g += [[0.5, 0.3 - 20 * h, 0.0, 0.37 * h, n], [0.5 - 30 * h, 0.3, 0.41 * h, 0.0, n], [0.5 + 25 * h, 0.3 + 25 * h, -0.33 * h, -0.29 * h, n],
              [0.5 - 9 * h, 0.3 + 13 * h, 0.9 * h, -0.7 * h, n], [0.5, 0.3, 0.0, 0.0, n], [0.5, 0.3, -0.0, 0.0, n], [0.5, 0.3, 0.0, -0.21 * h, n]]
    # across the whole u16 domain and out of it on both sides (saturated cells at either end)
    lo, hi = float(gmin[0]) - 40 * h, float(gmin[0]) + 65600 * h
    g += [[lo, 0.3, (hi - lo) / 400, 0.0, 401], [hi, 0.3, -(hi - lo) / 400, 0.0, 401], [0.5, float(gmin[1]) - 3 * h, 0.0, 66000 * h / 250, 251],
          [lo, float(gmin[1]) + 65600 * h, (hi - lo) / 300, -(hi - lo) / 300, 301]]
    # steps so large that k * d or the sum overflows
    g += [[0.5, 0.3, 1e38, 0.0, 9], [0.5, 0.3, -1e38, 3e38, 9], [3e38, -3e38, 3e38, -3e38, 7], [-3e38, 0.3, 3.4e38, 1e-30, 5], [0.5, 0.3, 1e-40, -1e-40, 50]]
    return g


@pytest.mark.parametrize("grid", ["app", "fine", "tiny", "odd"])
def test_owned_samples_are_one_interval_and_the_bisection_finds_it(driver, grid):
    gmin, inv = grid_of(grid)
    gauges = y._gauge_array(rays(gmin, inv))
    rows = gr.gauge_rows(rays(gmin, inv))
    for name, rects in tilings(gmin, inv).items():
        payload = np.array([gmin[0], gmin[1], inv], F).tobytes() + np.array([len(rects), len(gauges)], np.uint32).tobytes() + \
            np.array(rects, np.uint32).tobytes() + gauges.tobytes()
        _, got = driver("window", payload, np.uint32)
        got = got.reshape(len(rects), len(gauges), 2).astype(np.int64)
        split = 0
        for k, g in enumerate(rows):
            want = gmr.intervals(g, gmin, inv, rects)  # (asserts: contiguous, every sample owned exactly once)
            assert np.array_equal(got[:, k], want), (grid, name, k, g, got[:, k], want)
            split += (want[:, 1] > 0).sum() > 1
        assert split >= 8, (grid, name, split)  # the cuts really pass through rays


# ------------------------------------------------------------------------------------------------------------- the fold
def value_arrays():
    """seeded (n, values, what): profiles, noise, nothing inside, everything inside, NaNs; n from 1 to 200"""
    rng = np.random.default_rng(20)
    out = []
    for n in list(range(1, 41)) + [63, 64, 65, 127, 128, 129, 199, 200]:
        prof = (np.clip(1.15 - np.arange(n) / max(n * rng.uniform(0.2, 1.2), 1.0), 0, 1) + rng.normal(0, 0.05, n)).astype(F)
        out.append((n, prof, "profile"))
        out.append((n, rng.random(n, dtype=F), "noise"))
        nan = rng.random(n, dtype=F)
        nan[rng.random(n) < 0.3] = NAN
        out.append((n, nan, "NaNs"))
        if n % 7 == 1:
            out.append((n, (rng.random(n, dtype=F) * F(0.4)).astype(F), "nothing inside"))
            out.append((n, (rng.random(n, dtype=F) + F(0.5)).astype(F), "everything inside"))
            end = rng.random(n, dtype=F) * F(0.4)
            end[-1] = F(0.9)
            out.append((n, end.astype(F), "last == n-1"))
    return out


def splits(n, last, rng):
    """cut lists 0 = c0 <= ... <= cp = n for 1 to 5 intervals: random ones, `last` at an interval's end (a cut at last + 1), a cut on both
    sides of `last`, and repeated cuts (empty parts)"""
    out = [[0, n]]
    for parts in (2, 3, 4, 5):
        for _ in range(3):
            out.append([0] + sorted(int(v) for v in rng.integers(0, n + 1, parts - 1)) + [n])
        if last is not None:
            others = sorted(int(v) for v in rng.integers(0, n + 1, parts - 2))
            out.append(sorted([0, last + 1] + others) + [n])
            if parts >= 3:
                out.append(sorted([0, last, last + 1] + others[:parts - 3]) + [n])
    out.append([0, 0, n, n])
    out.append([0, n // 2, n // 2, n // 2, n])
    return out


def test_fold_equals_the_rule_over_the_concatenated_values(driver, sphx_lib):
    rng = np.random.default_rng(21)
    gauges, parts_rows, wants, seen = [], [], [], set()
    for n, f, what in value_arrays():
        g = (F(0.1), F(0.7), F(0.003), F(-0.007), n)
        want = gr.reduce_one(g, f, 0.5)
        last = None if want["last"] == gr.NONE else int(want["last"])
        for cuts in splits(n, last, rng):
            parts = gmr.parts_of(f, cuts, 0.5)
            parts = parts[rng.permutation(len(parts))]  # the fold orders them itself
            assert gmr.same_bytes(gmr.fold(g, 0.5, parts), want), (what, n, cuts)
            if last is not None and last + 1 < n and last + 1 in cuts:
                seen.add("last ends an interval")
            if last == n - 1:
                seen.add("last == n-1")
            if last is None:
                seen.add("nothing inside")
            if len(set(cuts)) < len(cuts):
                seen.add("empty parts")
            pad = np.zeros(5, gmr.PART_DTYPE)  # for the header and the library: five parts per gauge, shorter lists padded with empty parts
            pad[:len(parts)] = parts
            for q in pad[len(parts):]:
                q["first"] = q["last"] = gr.NONE
            gauges.append(list(g))
            parts_rows.append(pad)
            wants.append(want)
    assert seen == {"last ends an interval", "last == n-1", "nothing inside", "empty parts"}
    # the same cases through sphx_gauge_merge.hpp compiled alone, and through the library: parts[p][gauge]
    G = y._gauge_array(gauges)
    P = np.ascontiguousarray(np.stack(parts_rows, 1))  # [5, gauges]
    W = np.array(wants, gr.REC_DTYPE)
    for lo in range(0, len(G), 1000):
        sl = slice(lo, min(lo + 1000, len(G)))
        got = y.gauge_merge(np.ascontiguousarray(P[:, sl]), G[sl], 0.5)
        assert gmr.same_bytes(got, W[sl])
        payload = np.array([len(G[sl])], np.uint32).tobytes() + np.array([0.5], F).tobytes() + np.array([5], np.uint32).tobytes() + G[sl].tobytes() + \
            np.ascontiguousarray(P[:, sl]).tobytes()
        out, rec = driver("fold", payload, gr.REC_DTYPE)
        assert out.split()[1] == "0" and gmr.same_bytes(rec, W[sl]), out


def test_mutants_of_the_fold_are_rejected():
    """f_next taken from the owner of `last` alone, max for first, a fold that ignores the counts: each differs from the rule on some split"""
    rng = np.random.default_rng(22)
    killed = {v: 0 for v in gmr.VARIANTS[1:]}
    for n, f, what in value_arrays():
        g = (F(0.1), F(0.7), F(0.003), F(-0.007), n)
        want = gr.reduce_one(g, f, 0.5)
        last = None if want["last"] == gr.NONE else int(want["last"])
        for cuts in splits(n, last, rng):
            parts = gmr.parts_of(f, cuts, 0.5)
            for v in ("next_from_owner_only", "max_for_first"):
                killed[v] += not gmr.same_bytes(gmr.fold(g, 0.5, parts, v), want)
            # a tile that lost its last sample (a count below the interval): the contract refuses, the mutant returns a record
            big = [k for k in range(len(parts)) if parts[k]["count"] > 1]
            if big:
                bad = parts.copy()
                bad[big[0]] = gmr.part_of(f, int(bad[big[0]]["lo"]), int(bad[big[0]]["count"]) - 1, 0.5)
                with pytest.raises(gmr.Refused):
                    gmr.fold(g, 0.5, bad)
                gmr.fold(g, 0.5, bad, "ignore_count")
                killed["ignore_count"] += 1
    assert all(v > 20 for v in killed.values()), killed


# ------------------------------------------------------------------------------------------------------------- refusals
def test_fold_refuses_a_gap_an_overlap_and_a_wrong_count(driver, sphx_lib):
    n = 50
    f = np.clip(1.1 - np.arange(n) / 30.0, 0, 1).astype(F)
    g = [0.1, 0.7, 0.003, -0.007, n]
    row = gr.gauge_rows([g])[0]
    good = gmr.parts_of(f, [0, 17, 31, n], 0.5)
    want = gr.reduce_one(row, f, 0.5)
    assert gmr.same_bytes(y.gauge_merge(good, [g], 0.5), want)
    cases = {}
    cases["gap"] = np.array([gmr.part_of(f, 0, 17, 0.5), gmr.part_of(f, 18, 13, 0.5), gmr.part_of(f, 31, 19, 0.5)], gmr.PART_DTYPE)
    cases["gap at the end"] = good[:2]
    cases["overlap"] = np.array([gmr.part_of(f, 0, 17, 0.5), gmr.part_of(f, 16, 15, 0.5), gmr.part_of(f, 31, 19, 0.5)], gmr.PART_DTYPE)
    cases["a sample owned twice"] = np.concatenate([good, good[1:2]])
    low = good.copy()
    low[1]["count"] -= 1  # the device accepted one sample less than the host's interval
    cases["count too low"] = low
    high = good.copy()
    high[0]["count"] += 1
    cases["count too high"] = high
    behind = good.copy()
    behind[2]["count"] += 1
    cases["behind the ray"] = behind
    cases["no parts"] = good[:0]
    for name, parts in cases.items():
        with pytest.raises(gmr.Refused):
            gmr.fold(row, 0.5, parts)
        rec = np.full(1, 0x5A, np.uint8).repeat(32).view(y.GAUGE_REC_DTYPE)
        G = y._gauge_array([g])
        P = np.ascontiguousarray(parts, y.GAUGE_PART_DTYPE)
        rc = sphx_lib.sphx_gauge_merge(G.ctypes.data, 1, 0.5, P.ctypes.data if len(P) else None, len(P), rec.ctypes.data)
        assert rc == _lib.ERR_INVALID_ARGUMENT and (rec.view(np.uint8) == 0x5A).all(), name  # it never returns a record
        assert sphx_lib.sphx_multi_last_error(None).decode().startswith("sphx_gauge_merge: "), name
        with pytest.raises(y.SphxError):
            y.gauge_merge(parts, [g], 0.5)
        payload = np.array([1], np.uint32).tobytes() + np.array([0.5], F).tobytes() + np.array([len(P)], np.uint32).tobytes() + G.tobytes() + P.tobytes()
        out, raw = driver("fold", payload, np.uint8)
        assert out.split()[1] == "1" and (raw == 0xAB).all(), (name, out)
    # argument errors of the merge call
    rec = np.zeros(1, y.GAUGE_REC_DTYPE)
    G = y._gauge_array([g])
    P = np.ascontiguousarray(good, y.GAUGE_PART_DTYPE)
    assert sphx_lib.sphx_gauge_merge(G.ctypes.data, 1, 0.5, P.ctypes.data, 3, None) == _lib.ERR_INVALID_ARGUMENT
    assert sphx_lib.sphx_gauge_merge(None, 1, 0.5, P.ctypes.data, 3, rec.ctypes.data) == _lib.ERR_INVALID_ARGUMENT
    assert sphx_lib.sphx_gauge_merge(G.ctypes.data, 1, float("nan"), P.ctypes.data, 3, rec.ctypes.data) == _lib.ERR_INVALID_ARGUMENT
    assert sphx_lib.sphx_gauge_merge(G.ctypes.data, 1, 0.5, None, 3, rec.ctypes.data) == _lib.ERR_INVALID_ARGUMENT
    assert sphx_lib.sphx_gauge_merge(None, 0, 0.5, None, 0, rec.ctypes.data) == _lib.OK  # no gauges: nothing to fold
