"""Emitting and draining fluid in a tiled run (sphx_multi_append / sphx_multi_remove and the tile seam; include/sphx.h), the parts that
need no GPU: the header, the exports, the bindings and the NULL refusals; the reference's edit of a checkpoint part
(tests/multi_edit_reference.py) on a part built by hand; and the host rules — routing, id counter, position check
(yasph2d_amd/csrc/sphx_multi_edit.hpp) — as a stand-alone program built with the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import multi_edit_reference as xref
import multi_state_reference as mref
import state_reference as sref
import yasph2d_amd as y
from yasph2d_amd import _lib
from yasph2d_amd.multi import MultiSolver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "yasph2d_amd", "csrc")
CALLS = ("sphx_multi_append", "sphx_multi_remove", "sphx_tile_remove_mark", "sphx_tile_remove_fetch", "sphx_tile_append")


# ------------------------------------------------------------------------------------------------------ 1. header, exports, bindings, NULL
def test_symbols_exported_and_declared(sphx_lib):
    full = open(os.path.join(ROOT, "include", "sphx.h")).read()
    src = re.sub(r"/\*.*?\*/", "", full, flags=re.S)
    for name in CALLS + ("sphx_tile_grow",):
        assert re.search(r"\bint\s+%s\s*\(" % name, src), f"{name} is not declared in include/sphx.h"
        assert hasattr(sphx_lib, name), f"{name} is not exported by libsphx.so"
        assert name in _lib.SIGNATURES, name
    assert "SPHX_ABI_VERSION 5" in src and sphx_lib.sphx_abi_version() == 5  # additions only
    assert re.search(r"5 \(additive\): sphx_multi_append, sphx_multi_remove", full)
    # the single context's section points at the new one instead of saying that a tiled run has no counterpart
    single = full.split("---- emitting and draining fluid: the particle set edited on the device")[1].split("typedef struct sphx_rect")[0]
    assert "no counterpart" not in single and "sphx_multi_append / sphx_multi_remove" in single
    tiled = full.split("---- emitting and draining fluid in a tiled run")[1].split("int sphx_multi_append")[0]
    for needle in ("COLLECTIVE", "all-reduce", "decided from it alone", "exchanges grows by exactly 1", "not counted", "first_id + k",
                   "1 + the greatest id", "2^31", "never reused within a run that does not load", "CURRENT layout", "kappa = stiffness = +0.0",
                   "grows its arrays by half", "n_new == 0", "borrowed", "No flag is raised", "sphx_multi_state_save", "bit-identical",
                   "SPHX_ERR_NOT_READY", "cap_records", "12 bytes per local record"):
        assert needle in tiled, needle
    for method in ("append", "remove"):
        assert hasattr(MultiSolver, method) and hasattr(y.DFSPHMultiSolver, method), method


def test_null_arguments_are_refused(sphx_lib):
    L, bad = sphx_lib, _lib.ERR_INVALID_ARGUMENT
    one = (_lib.SphxRect * 1)(_lib.SphxRect(0, 0, 1, 1))
    xy = np.float32([[0.5, 0.5]])
    ids = np.uint32([7])
    first, removed, owned = C.c_uint32(123), C.c_uint64(456), C.c_uint32(789)
    assert L.sphx_multi_append(None, xy.ctypes.data, None, 1, C.byref(first)) == bad and L.sphx_multi_append(None, None, None, 0, None) == bad
    assert L.sphx_multi_remove(None, one, 1, 0, C.byref(removed)) == bad and L.sphx_multi_remove(None, None, 0, 0, None) == bad
    assert L.sphx_tile_remove_mark(None, one, 1, 0) == bad and L.sphx_tile_remove_fetch(None, C.byref(owned)) == bad
    assert L.sphx_tile_append(None, xy.ctypes.data, None, ids.ctypes.data, 1) == bad and L.sphx_tile_grow(None, 10) == bad
    assert (first.value, removed.value, owned.value) == (123, 456, 789)  # nothing was written


# ------------------------------------------------------------------------------------------------------ 2. the reference's edit of a part
def hand_part(n=5, b=3, ids=(4, 0, 9, 2, 7)):
    """One part of a 2 x 2 run, packed field by field from the layout comment of sphx_multi_state_format.hpp."""
    rng = np.random.default_rng(5)
    ids = np.array(ids[:n], "<u4")
    sec = dict(positions=rng.random((n, 2), np.float32), velocities=rng.random((n, 2), np.float32) - 0.5, particle_id=ids,
               density=rng.random(n, np.float32) + 100, alpha=rng.random(n, np.float32), kappa=-rng.random(n, np.float32), stiffness=rng.random(n, np.float32),
               boundary=rng.random((b, 2), np.float32))
    head = bytearray(mref.HEADER_BYTES)
    head[0:8] = b"SPHXMULT"
    struct.pack_into("<II", head, 8, 1, 0x01020304)
    struct.pack_into("<IIII", head, 24, mref.HEADER_BYTES, len(mref.SECTIONS), mref.PARAMS_BYTES, 0)
    p = y.default_params()
    p.device = 0
    head[mref.PARAMS_AT:mref.PARAMS_AT + mref.PARAMS_BYTES] = bytes(p)
    struct.pack_into("<Q", head, 120, n)
    struct.pack_into("<IIII", head, 128, n, b, 0, 1)
    struct.pack_into("<IIII", head, 144, 3, 2, 2, 1)
    struct.pack_into("<Q", head, 160, 40)
    struct.pack_into("<II", head, 168, 1, 4)
    cuts = [0, 40, 65536, 0, 17, 65536, 0, 23, 65536]
    struct.pack_into("<iIII", head, 176, -1, 2, 2, len(cuts))
    struct.pack_into("<%dI" % len(cuts), head, mref.CUTS_AT, *cuts)
    body, at = bytearray(), mref.HEADER_BYTES
    for s, name in enumerate(mref.SECTIONS):
        data = np.ascontiguousarray(sec[name]).tobytes()
        dig = sref.digest(sec[name]) if name == "boundary" else mref.digest_by_id(ids, sec[name])
        struct.pack_into("<QQQ", head, mref.TABLE_AT + 24 * s, at, len(data), dig)
        body += data + b"\0" * ((-len(data)) % 8)
        at += len(data) + (-len(data)) % 8
    struct.pack_into("<Q", head, 16, at)
    struct.pack_into("<Q", head, mref.DIGEST_AT, sref.digest(bytes(head[:mref.DIGEST_AT])))
    return bytes(head) + bytes(body), sec


@pytest.mark.parametrize("n", [5, 4, 1, 0])
def test_edit_part_of_an_unedited_part_is_the_part(n):
    blob, _ = hand_part(n)
    mref.parse_part(blob)  # (the hand-made part is one the parser accepts)
    assert xref.edit_part(blob) == blob
    assert xref.edit_part(blob, keep_mask=np.ones(n, bool), appended=(np.zeros((0, 2)), None, np.zeros(0))) == blob


def test_edit_part_drops_and_adds():
    blob, sec = hand_part()
    keep = np.array([True, False, True, True, False])
    new_pos, new_ids = np.float32([[0.25, 0.5], [0.75, 0.125]]), np.uint32([10, 11])
    p = mref.parse_part(xref.edit_part(blob, keep_mask=keep, appended=(new_pos, None, new_ids)))
    assert (p["n_total"], p["n_part"], p["b"], p["steps"], p["num_density_iters"], p["cuts"]) == (5, 5, 3, 40, 3, [0, 40, 65536, 0, 17, 65536, 0, 23, 65536])
    assert p["particle_id"].tolist() == [4, 9, 2, 10, 11]
    assert p["positions"].tobytes() == np.concatenate([sec["positions"][keep], new_pos]).tobytes()
    zero2 = np.zeros(2, np.float32).tobytes()  # +0.0: all bits clear
    for name in ("kappa", "stiffness", "density", "alpha"):
        assert p[name][:3].tobytes() == sec[name][keep].tobytes() and p[name][3:].tobytes() == zero2, name
    assert p["velocities"][3:].tobytes() == np.zeros((2, 2), np.float32).tobytes() and p["boundary"].tobytes() == sec["boundary"].tobytes()
    for name in mref.SECTIONS[:7]:  # the id-keyed digests, in Python integers
        rows = np.frombuffer(p[name].tobytes(), "<u4").reshape(5, -1)
        assert p["table"][name][2] == mref.digest_by_id_ints(p["particle_id"].tolist(), rows.tolist()), name
    # a part of several: the caller gives the run's new total
    assert mref.parse_part(xref.edit_part(blob, keep_mask=keep, n_total=3))["n_total"] == 3
    # everything removed
    e = mref.parse_part(xref.edit_part(blob, keep_mask=np.zeros(5, bool)))
    assert (e["n_total"], e["n_part"]) == (0, 0) and e["total_bytes"] == mref.HEADER_BYTES + 8 * 3


def test_id_counter_rule_restated():
    assert xref.counter_after(None, 4050) == 4050 and xref.counter_after([7, 3, 1000, 12], 4) == 1001 and xref.counter_after([], 0) == 0
    assert xref.take_ids(4050, 81) == (4050, 4131) and xref.take_ids((1 << 31) - 2, 2) == ((1 << 31) - 2, 1 << 31)
    assert xref.take_ids((1 << 31) - 2, 3) is None and xref.take_ids(1 << 31, 1) is None


# ------------------------------------------------------------------------------------------------------ 3. the host rules, under sanitizers
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to compile the multi-edit driver"
    exe = str(tmp_path_factory.mktemp("multi_edit") / "multi_edit_driver")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(ROOT, "tests", "multi_edit_driver.cpp"), "-o", exe])

    def run(*args):
        r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
        return r.returncode, r.stdout, r.stderr

    return run


@pytest.mark.parametrize("check", ["routing", "ids", "positions", "empty"])
def test_host_rules(driver, check):
    """routing: strips and a 2 x 2 grid against hand cases — a record exactly on a cut, records in the corner cells, rectangles with a gap,
    order independence.  ids: NULL ids, explicit ids with gaps, the overflow at 2^31.  positions: NaN / +-inf in either coordinate at any
    record.  empty: n_new == 0.  The sanitizers stay clean (any report aborts the program)."""
    rc, out, err = driver(check)
    assert rc == 0 and out.startswith("ok ") and err == "", (out[-2000:], err[-2000:])
    assert int(out.split()[1]) > 0


def test_header_has_no_hip():
    src = open(os.path.join(CSRC, "sphx_multi_edit.hpp")).read()
    assert "hip" not in "".join(re.findall(r"#include\s*[<\"]([^>\"]+)", src)).lower()


def test_numpy_routing_equals_the_header(driver):
    """The restated routing rule (multi_edit_reference.route over layout_rects of a parsed part) against the C++ on random records around
    the cuts of the hand-made part's 2 x 2 layout, cuts and corner cells included."""
    p = mref.parse_part(hand_part()[0])
    rects = xref.layout_rects(p)
    assert rects == [(0, 40, 0, 17), (0, 40, 17, 65536), (40, 65536, 0, 23), (40, 65536, 23, 65536)]
    rng = np.random.default_rng(3)
    cells = np.concatenate([rng.integers(0, 80, (300, 2)), [[0, 0], [0, 65535], [65535, 0], [65535, 65535], [40, 17], [39, 17], [40, 23], [40, 22], [39, 16]]])
    h, gmin = np.float32(0.02), np.float32(-100.0)
    pos = (gmin + (cells.astype(np.float32) + rng.random(cells.shape, np.float32) * np.float32(0.9) + np.float32(0.05)) * h).astype(np.float32)
    own = xref.route(pos, rects, (gmin, gmin), h)
    args = [repr(float(gmin)), repr(float(h)), len(rects)] + [v for r in rects for v in r] + [repr(float(v)) for v in pos.reshape(-1)]
    rc, out, err = driver("route", *args)
    assert rc == 0 and err == "", err[-2000:]
    assert [int(v) for v in out.split()] == own.tolist()
    assert set(own.tolist()) == {0, 1, 2, 3}
