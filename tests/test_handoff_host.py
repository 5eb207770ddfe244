"""The hand-off records of the host step path (yasph2d_amd/csrc/sphx_handoff.hpp) against the loose context members they replaced:
tests/handoff_driver.cpp restates those members and every statement that touched them as the model, drives model and records through
every sequence of up to six host-side events and compares, after every event, everything a consumer is told.  A sanitized stand-alone
program; needs no GPU."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "yasph2d_amd", "csrc")
REMOVED = ("div_error_fused", "div_warm_fused", "div_knz_fused", "div_mark_tag", "div_warm_taken", "count_done", "count_n", "count_from_class",
           "tile_class_done", "tile_class_n", "tile_class_dt_bits", "fuse_count_ok")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to compile the hand-off driver"
    exe = str(tmp_path_factory.mktemp("handoff") / "handoff_driver")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, os.path.join(ROOT, "tests", "handoff_driver.cpp"), "-o", exe])

    def run(*args):
        r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
        return r.returncode, r.stdout, r.stderr

    return run


@pytest.mark.parametrize("record, events", [("build", 18), ("count", 16)])
def test_records_tell_consumers_what_the_flags_told_them(driver, record, events):
    """build: BuildHandoff — neighbour builds of the four kinds (with and without flags and take-over, one over zero particles), the
    single context's iterations, the tile sub-steps, the failure path and sphx_state_load.  count: PendingCount — counting and
    classifying corrections, packs, sphx_tile_count_kept, builds, the drops, the entry points that only bar the take-over, a new
    directory; from a plain context and from a tile.  Every sequence up to length 6, every answer equal, the sanitizers clean."""
    rc, out, err = driver(record)
    assert rc == 0 and out.startswith("ok ") and err == "", (out[-2000:], err[-2000:])
    sequences, checks = (int(x) for x in out.split()[1:3])
    starts = 2 if record == "count" else 1
    assert sequences == checks == starts * sum(events ** k for k in range(1, 7))


def test_driver_plumbing(driver):
    """The driver's own plumbing: unknown checks and depths are refused, a shallow walk counts what it should."""
    assert driver("build", 2)[1].split()[:2] == ["ok", str(18 + 18 * 18)]
    assert driver("nonsense")[0] == 2 and driver("build", 0)[0] == 2


def test_the_loose_members_are_gone():
    """None of the members the records replaced is named in the library's sources or the tools any more."""
    pat = re.compile(r"\b(" + "|".join(REMOVED) + r")\b")
    hits = []
    for d in (CSRC, os.path.join(ROOT, "tools")):
        for name in sorted(os.listdir(d)):
            path = os.path.join(d, name)
            if os.path.isfile(path) and not name.endswith((".o", ".so")):
                with open(path, errors="replace") as f:
                    hits += ["%s:%d" % (name, k + 1) for k, line in enumerate(f) if pat.search(line)]
    assert not hits, hits
