"""Following particles by id (sphx_track_*, sphx_download_by_id, include/sphx.h), the parts that need no GPU: the numpy reference on
hand cases, the host half of a tracked set as a sanitized stand-alone program, and the exports / bindings / NULL handling / harness
options."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import track_reference as ref

from yasph2d_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "yasph2d_amd", "csrc")
TRACK_CALLS = ("sphx_track_set", "sphx_track_fetch", "sphx_track_record", "sphx_track_get_status", "sphx_track_read", "sphx_download_by_id")
A, W = int(ref.ABSENT), int(ref.ABSENT_WORD)


# ------------------------------------------------------------------------------------------------------ 1. the reference
def test_reference_hand_cases():
    f = lambda *v: np.array(v, np.float32)  # noqa: E731
    d = {"ids": np.array([7, 3, 9, 3], np.uint32), "pos": np.array([[0, 1], [2, 3], [4, 5], [6, 7]], np.float32),
         "vel": np.array([[-0.0, 1], [np.nan, 3], [4, 5], [np.inf, -7]], np.float32), "density": f(10, 11, 12, 13)}
    assert ref.slot_of(d["ids"], [3, 7, 8, 9, 3]).tolist() == [3, 0, A, 2, 3]  # the HIGHEST slot of the repeated id 3
    r = ref.fetch(d, [9, 8, 3])
    assert r["slot"].tolist() == [2, A, 3]
    assert r["pos"].tolist() == [ref.words(f(4, 5)).tolist(), [W, W], ref.words(f(6, 7)).tolist()]
    assert r["vel"].tolist() == [ref.words(f(4, 5)).tolist(), [W, W], ref.words(f(np.inf, -7)).tolist()]
    assert r["density"].tolist() == [ref.words(f(12))[0], W, ref.words(f(13))[0]]
    # the absent word is a quiet NaN; signed zeros and NaN payloads travel as bits
    assert np.isnan(np.array([W], np.uint32).view(np.float32)[0])
    assert ref.fetch(d, [7])["vel"][0, 0] == 0x80000000
    out, present = ref.by_id(d, 6, 5)  # ids 6 .. 10
    assert out["slot"].tolist() == [A, 0, A, 2, A] and present == 2
    out, present = ref.by_id(d, 0xFFFFFFFE, 2)
    assert out["slot"].tolist() == [A, A] and present == 0
    assert ref.frame(d, [3, 8]).tolist() == [ref.words(f(6, 7, np.inf, -7)).tolist(), [W] * 4]
    # an empty context: everything absent; an empty set: empty outputs
    e = {"ids": np.zeros(0, np.uint32), "pos": np.zeros((0, 2), np.float32), "vel": np.zeros((0, 2), np.float32), "density": np.zeros(0, np.float32)}
    assert ref.fetch(e, [0, 1])["slot"].tolist() == [A, A] and ref.frame(e, [0]).tolist() == [[W] * 4]
    assert ref.fetch(d, [])["pos"].shape == (0, 2) and ref.by_id(d, 3, 0)[1] == 0


# ------------------------------------------------------------------------------------------------------ 2. the tracked set's host half
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to compile the tracked-set driver"
    exe = str(tmp_path_factory.mktemp("track_set") / "track_set_driver")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, os.path.join(ROOT, "tests", "track_set_driver.cpp"), "-o", exe])

    def run(*args):
        r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
        return r.returncode, r.stdout, r.stderr

    return run


@pytest.mark.parametrize("check", ["empty", "one", "duplicates", "maximum", "extremes", "filter", "checks"])
def test_track_set_host(driver, check):
    """empty: the empty set.  one: a single id.  duplicates: all ids equal, and repeats among others.  maximum: SPHX_TRACK_MAX_IDS ids
    (consecutive, random, descending).  extremes: the ids 0 and 0xFFFFFFFF.  filter: every member of every set passes the filter, and
    few others do.  checks: the argument checks.  The sanitizers stay clean (any report aborts the program)."""
    rc, out, err = driver(check)
    assert rc == 0 and out.startswith("ok ") and err == "", (out[-2000:], err[-2000:])
    assert int(out.split()[1]) > 0


def test_track_set_header_has_no_hip():
    src = open(os.path.join(CSRC, "sphx_track_set.hpp")).read()
    assert "hip" not in "".join(re.findall(r"#include\s*[<\"]([^>\"]+)", src)).lower()


# ------------------------------------------------------------------------------------------------------ 3. exports, bindings, NULL, harness
def test_header_declares_and_library_exports(sphx_lib):
    full = open(os.path.join(ROOT, "include", "sphx.h")).read()
    src = re.sub(r"/\*.*?\*/", "", full, flags=re.S)
    for name in TRACK_CALLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, src), f"{name} is not declared in include/sphx.h"
        assert hasattr(sphx_lib, name), f"{name} is not exported by libsphx.so"
        assert name in _lib.SIGNATURES
    assert re.search(r"#define\s+SPHX_TRACK_MAX_IDS\s+16384\b", src) and re.search(r"#define\s+SPHX_TRACK_ABSENT\s+0xFFFFFFFFu", src)
    assert re.search(r"SPHX_TRACK_DEVICE_POINTERS\s*=\s*1u", src) and "SPHX_ABI_VERSION 5" in src
    assert (_lib.TRACK_MAX_IDS, _lib.TRACK_ABSENT, _lib.TRACK_ABSENT_WORD, _lib.TRACK_DEVICE_POINTERS) == (16384, A, W, 1)
    assert C.sizeof(_lib.SphxTrackOut) == 4 * C.sizeof(C.c_void_p) and C.sizeof(_lib.SphxTrackStatus) == 32
    # the header lists the calls as STABLE, says what the absent word is and that sphx_multi_* has no counterpart
    assert "sphx_track_*, sphx_download_by_id" in full.split("INSPECTION")[0]
    assert "0x7FC00000" in full and len(re.findall(r"sphx_multi_\* has NO counterpart", full)) >= 2


def test_null_arguments_are_refused(sphx_lib):
    L, bad = sphx_lib, _lib.ERR_INVALID_ARGUMENT
    ids = (C.c_uint32 * 4)(1, 2, 3, 4)
    buf = (C.c_float * 64)()
    o = _lib.SphxTrackOut(C.addressof(buf), None, None, None)
    st = _lib.SphxTrackStatus()
    n = C.c_uint32(123)
    assert L.sphx_track_set(None, ids, 4) == bad and L.sphx_track_set(None, None, 0) == bad
    assert L.sphx_track_fetch(None, 0, C.byref(o)) == bad and L.sphx_track_fetch(None, 0, None) == bad
    assert L.sphx_track_record(None, 10, 1) == bad and L.sphx_track_record(None, 0, 0) == bad
    assert L.sphx_track_get_status(None, C.byref(st)) == bad and L.sphx_track_get_status(None, None) == bad
    assert L.sphx_track_read(None, 0, 1, 0, buf) == bad and L.sphx_track_read(None, 0, 0, 0, None) == bad
    assert L.sphx_download_by_id(None, 0, 4, 0, C.byref(o), C.byref(n)) == bad and L.sphx_download_by_id(None, 0, 0, 0, None, None) == bad
    assert n.value == 123 and not any(buf)


def test_harness_help_names_the_options(sphx_lib):
    exe = os.path.join(ROOT, "yasph2d_amd", "sphx_harness")
    assert os.path.exists(exe), "sphx_harness is built by __graft_entry__.build()"
    r = subprocess.run([exe, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    assert "--track ID[,ID...]" in r.stdout and "--track-every E" in r.stdout and "--track-out FILE" in r.stdout
    for args in (["--track", "1,2"], ["--track-out", "x"], ["--track", "1,,2", "--track-out", "x"], ["--track", "-1", "--track-out", "x"],
                 ["--track", "1.5", "--track-out", "x"], ["--track", "4294967296", "--track-out", "x"],
                 ["--track", "1", "--track-every", "0", "--track-out", "x"], ["--track", "1", "--track-out"]):
        r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and "invalid --track" in r.stderr, (args, r.stderr)
